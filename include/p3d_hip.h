/* libp3dhip -- C ABI of the MI355X-native P3D saliency forward/backward path.
 *
 * The reference (A-Nasiri-M/sap3d_tensorflow) has no FFI layer: its boundary is the Python
 * graph function  p3d.p3d_unet(_X, _dropout, batch_size, training)  (reference p3d.py:169) plus
 * the tf.Session feed/fetch contract its drivers use (train.py:143-146,217-218,225-226;
 * gen_pred.py:45-46,151).  Each entry point below names the reference interface it replaces.
 * The binding a maintainer adds on the reference side is a ctypes stub; see INTEGRATION.md.
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on success and a
 * negative code on failure with the message available from p3d_last_error(); host buffers are
 * owned by the caller and copied by value (like feed_dict / fetched numpy arrays); device
 * memory, streams and RCCL state are owned by the opaque handle; one caller thread per handle
 * (like the single thread calling sess.run).  All tensors are float32 NDHWC.
 *
 * The Python binding is READ FROM THIS FILE (sap3d_tensorflow_amd/_header.py, at import): a declaration here is bound, and
 * nothing is written a second time.  The reader accepts this grammar and stops at anything else, naming it:
 *   block comments; #include, the include guard and the __cplusplus brackets; #define P3D_NAME <integer literal> (a #define
 *   with any other body is not a constant for Python); enum { A = n, ... }; with an explicit integer for every enumerator;
 *   typedef struct [tag] { ... } name; with several declarators per declaration (int ld, off; -- not after a pointer), fixed
 *   arrays, pointer members and earlier structs by value or in arrays; the opaque handle's typedef; function declarations with
 *   named parameters.
 * Types: int, float, double, char, unsigned char, size_t, void, [u]int32_t, [u]int64_t, p3d_handle and the structs defined
 * above their use, with const, up to two levels of pointer, and parameters name[N].  Scalars bind to their ctypes twins, a
 * void return to None, p3d_handle* and void* to c_void_p, [const] char* to c_char_p, any other T* to POINTER(T), a second
 * level (T**, T* const*, const char**, p3d_handle**) to POINTER of the first, a parameter T name[N] to POINTER(T), and
 * struct p3d_some_name to the ctypes.Structure P3dSomeName.
 */
#ifndef P3D_HIP_H
#define P3D_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct p3d_handle p3d_handle;

enum {
    P3D_STRUCTURE_UNET = 0,      /* train.py:149-150  --structure unet   -> p3d.p3d_unet   (p3d.py:169) */
    P3D_STRUCTURE_CONCAT = 1,    /* train.py:151-152  --structure concat -> p3d.p3d_concat (p3d.py:224), no sigmoid */
    P3D_STRUCTURE_GN_P3D = 2,    /* gn/train_p3d_gn_dataset.py:169-170 net='P3D' -> p3d_gn.inference_p3d (gn/p3d_gn.py:214):
                                    GroupNorm + CBAM on every residual, concat head, no sigmoid */
    P3D_STRUCTURE_UNETPP_NONSA = 3, /* p3d.p3d_unetplusplus_nonsa (p3d.py:401): the nested UNet++ head of
                                    train.py:153-154 `--structure unet++` with its attention blocks left out
                                    (layer wrappers utils/network.py:97-110) */
    P3D_STRUCTURE_GN_P3D_DECODER = 4, /* gn/train_p3d_gn_dataset.py:177-178 net='P3D_DECODER' ->
                                    p3d_gn.inference_p3d_decoder_block (gn/p3d_gn.py:489): GN/CBAM encoder, skip
                                    deconvs + concat, two conv-deconv-conv decoder blocks, 3x3x3 conv to 1 channel;
                                    variables live in scope "P3D/"; base must be a multiple of 16 */
    P3D_STRUCTURE_GN_P3D_CONCAT = 5, /* gn/train_p3d_gn_dataset.py:171-172 net='P3D_CONCAT' -> p3d_gn.inference_p3d_concat
                                    (gn/p3d_gn.py:279): GN_P3D with deconv_pool4 at 8*base instead of 16*base filters */
    P3D_STRUCTURE_UNETPP_DS = 6   /* p3d.p3d_unetplusplus_ds (p3d.py:340): the UNet++ head WITH self attention
                                    (utils/network.py:157-192) on x_4_0, x_3_1, x_2_2 and, keys/values pooled by 2,
                                    x_1_3.  (train.py:153-154 wires p3d_unetplusplus, p3d.py:280, whose last
                                    attention call adds tensors of different shapes and cannot be built.)
                                    base must be a multiple of 16 */
};

typedef struct p3d_config {
    int structure;        /* P3D_STRUCTURE_*                                                    */
    int batch;            /* clips per step on THIS device (placeholder dim 0, train.py:143)    */
    int frames;           /* 16 in the reference (train.py:139, p3d.py:5); multiple of 16        */
    int height, width;    /* 112 in the reference (p3d.py:4); multiples of 16                   */
    int base;             /* stem width; 64 in the reference (p3d.py:172,179,185,191)           */
    int blocks[3];        /* bottlenecks per stage; 3,8,36 in the reference (p3d.py:179,185,191) */
    int device;           /* HIP device ordinal (train.py:73 CUDA_VISIBLE_DEVICES=args.gpu)      */
    int world_size;       /* data-parallel replicas (1 = the reference's single device)          */
    int rank;
} p3d_config;

/* Fill *cfg with the reference architecture: unet, batch 2, 16x112x112, base 64, blocks 3/8/36. */
void p3d_default_config(p3d_config* cfg);

/* Builds the graph once, like the graph-construction part of train.py:143-172 / gen_pred.py:45-46. */
int p3d_create(const p3d_config* cfg, p3d_handle** out);
void p3d_destroy(p3d_handle* h);
const char* p3d_last_error(void);

/* ---- variables: tf.global_variables(), Saver var_list (train.py:180-185).  Names are the TF
 *      variable names (firstconv1, conv3_0_1, STA_0_2_S, STA_0_2_S_bias, dw3d_0,
 *      batch_normalization_7/gamma, .../moving_mean, conv3d_transpose/kernel, deconv1_bn/beta ...). */
int p3d_num_params(p3d_handle* h);
int p3d_param_info(p3d_handle* h, int index, const char** name, int* ndim, int64_t shape[5], int* trainable);
int p3d_set_param(p3d_handle* h, const char* name, const float* host, int64_t count);   /* saver.restore */
int p3d_get_param(p3d_handle* h, const char* name, float* host, int64_t count);         /* saver.save    */
int p3d_get_grad(p3d_handle* h, const char* name, float* host, int64_t count);          /* tf.gradients (parity hook) */
/* tf.global_variables_initializer (train.py:178): Xavier-uniform etc., SURVEY.md Appendix A.7. */
int p3d_init_params(p3d_handle* h, uint64_t seed);

/* ---- sess.run(pred, {x, dropout: 0, training: False})   train.py:225-226, gen_pred.py:151.
 *      x [B,T,H,W,3] -> pred [B,T,H,W,1].  `training` is the placeholder of train.py:145: it
 *      switches stem/decoder BN and dropout only; backbone BN always uses batch statistics
 *      (p3d.py:140,179,185,191).  Never updates moving statistics (UPDATE_OPS are not fetched).
 *
 *      THE DROPOUT MASK (with training and dropout_rate in (0, 1); part of the contract, and the same for p3d_train_step,
 *      p3d_backward and the *_device forms).  The structure's one dropout site holds an activation of `rows` = N*D*H*W rows of
 *      C channels; its element (row, c) has the dense index e = row * C + c, whatever row stride the buffer has.  In uint64
 *      arithmetic mod 2^64 (the SplitMix64 finaliser):
 *          z = seed + 0x9E3779B97F4A7C15 * (e + 1);
 *          z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;   z = (z ^ (z >> 27)) * 0x94D049BB133111EB;   z = z ^ (z >> 31);
 *          u01(seed, e) = float32(z >> 40) * 2^-24                      (24 bits, in [0, 1))
 *          keep(e) = u01(seed, e) >= dropout_rate                        (compared as float32)
 *      A kept element is multiplied by 1 / (1 - dropout_rate), formed in float32, a dropped one is 0, forward and backward alike.  The
 *      mask is this function of (seed, e) and nothing else: not of the launch shape, the path a pass takes, whether the seed is an
 *      argument or read from device memory (captured steps), the replica or the run.  tests/dropout_ref.py replays it. */
int p3d_forward(p3d_handle* h, const float* x, int training, float dropout_rate, uint64_t seed, float* pred);

/* ---- B sliding windows of gen_pred.py:100-168 in one pass.  The reference runs sess.run(pred, ...) once per
 *      window with a batch of ONE clip (gen_pred.py:45,151), so the backbone's batch-statistics BatchNorm
 *      (p3d.py:140) sees one clip at a time.  This entry point takes `batch` windows x [B,T,H,W,3] and returns for
 *      each exactly what a batch-of-1 p3d_forward(training=0, dropout=0) returns for it: every batch-statistics
 *      BN normalises each clip with that clip's own statistics.  (For the GroupNorm structures it equals
 *      p3d_forward, GN has no cross-clip coupling.) */
int p3d_predict_windows(p3d_handle* h, const float* x, float* pred);

/* ---- sess.run([train_op, loss], {x, y, dropout, training: True})   train.py:217-218.
 *      y [B,T,H,W]; the selected loss, Smooth-L1 by default (SUM, utils/network.py:49-62; p3d_set_loss), Adam on
 *      every trainable (train.py:168), BN moving-average updates (train.py:170-172).  With world_size > 1 the
 *      gradients are summed across replicas (RCCL) before Adam.  The dropout mask is the function of (seed, element)
 *      defined at p3d_forward. */
int p3d_train_step(p3d_handle* h, const float* x, const float* y, float dropout_rate, uint64_t seed, float* loss);

/* ---- Non-finite values (NaN, +inf, -inf) in inputs, activations, gradients and weights.  A corrupt frame must show in the
 *      loss, not train the network on zeros; tests/test_gpu_nonfinite.py holds every kernel to the six items below.
 *   1. Forward kernels propagate.  An output is NaN exactly where the float64 reference of the same operation is NaN, and
 *      nowhere else; the same holds for +inf and for -inf.  The reference is written with propagating primitives:
 *      relu(v) = v > 0 ? v : (v != v ? v : 0) (numpy's maximum, not fmaxf, which returns the operand that is not NaN), a
 *      max-pool window -- CBAM's pools over positions and over channels included -- that holds a NaN gives NaN, a variance
 *      that is NaN stays NaN under its clamp at 0, and every sum is a sum.
 *   2. Finite values.  Outside that footprint every result is finite, and where the operation couples nothing across the
 *      poisoned element it has the BITS of the same launch on clean data: the other samples under GroupNorm and CBAM, the
 *      other channels under BatchNorm, the other maps in the per-map losses, the other elements in the optimisers, the moving
 *      average and the accumulation kernel, positions outside a convolution's receptive field, the other members of a
 *      grouped launch.  Every finite value gives the bits it gave before this paragraph existed, and relu(-0.f) is +0.f.
 *   3. max-pool arg-max: the first NaN tap in (kd, kh, kw) scan order if the window holds one, otherwise the first maximum
 *      (for a window of nothing but -inf: its first tap inside the tensor).  Both backward kernels send the gradient there.
 *   4. ReLU gates in the backward pass are selects: pre > 0 ? g : 0, so a NaN pre-activation has a closed gate and passes no
 *      gradient (references use where(mask, g, 0), never g * mask).  The poison reaches the gradients through the loss, which
 *      item 1 makes NaN, and through the statistics sums.
 *   5. The fp16 pointwise mode (p3d_set_pointwise_fp16) is held to the same rule for NaN and +-inf among operands of
 *      magnitude below 4; finite values that overflow fp16 are not part of this contract.
 *   6. Infinite weights are outside the contract (SAME padding multiplies zeros by the weight, so 0 * inf at the borders is
 *      an implementation detail).  NaN weights are inside: a NaN in a tap that lies inside the tensor at every output
 *      position (the centre tap) makes output channel co NaN at every position.  In the same way the head's filter gradients
 *      multiply x by the zero gradient of output positions past the border: a NaN or inf x in a border cell also reaches the
 *      taps of its channel that never read it (that channel's gradient is non-finite either way).
 *      Not part of the contract: stopping a training run on a non-finite loss (drivers/train.py reports the loss). */

/* Parity hook: forward (training=True) + the selected loss (Smooth-L1 by default) + backward, no Adam, no moving-stat update.
 * pred may be NULL.  Gradients are then readable with p3d_get_grad. */
int p3d_backward(p3d_handle* h, const float* x, const float* y, float dropout_rate, uint64_t seed,
                 float* loss, float* pred);

/* BASELINE.json configs[4] ("fp16 MFMA pointwise convs"; no reference counterpart, the reference is fp32 throughout):
 * when enabled, every 1x1x1 convolution (forward and input gradient) rounds its operands to fp16 in registers and
 * multiplies on the fp16 matrix cores with fp32 accumulation.  Everything stored stays fp32.  Parity for this mode is
 * fp16-level (2e-2 relative on the saliency maps); the default, fp32, is the mode the 1e-3 target applies to. */
int p3d_set_pointwise_fp16(p3d_handle* h, int enable);

/* BatchNorm fusion (no reference counterpart: an execution choice, the arithmetic is tf.layers.batch_normalization's either
 * way, p3d.py:56-81,88-97).  When on, the bn -> relu pairs between the convs of a small-tensor bottleneck are applied on the
 * operand paths of the neighbouring convolutions and never stored (fewer launches; measured no faster on one MI355X at 8
 * clips, so the default is off).  enable = 0: every BatchNorm is a pass of its own (the
 * round-2 launch list); 1: the forward pass is fused, BatchNorm's backward keeps its launches (the filter gradients read
 * the never-stored activations through the transform); 2: the backward pass is fused as well. */
int p3d_set_bn_fusion(p3d_handle* h, int enable);

/* The core of attention(), softmax(g f^T) h (utils/network.py:183-185; p3d_unetplusplus_ds, p3d.py:340-397) -- an execution
 * choice, the arithmetic is the reference's either way (only the order of the sums differs):
 *   1  three GEMMs per direction around a stored [N_g x N_f] score matrix and attention map (2 x B*N_g*N_f floats per block);
 *   2  score tiles recomputed on chip, nothing of size N_g x N_f in HBM (blocks of 32, 64, 128 or 256 channels; wider ones
 *      keep the GEMMs) -- the only way the last block fits at 8 clips of 32x224x224 (B*N_g*N_f = 5e10);
 *   0  (default) per block: 2 where the score matrix has 2^24 elements or more, else 1.
 * Switching to 1 allocates the score buffers of blocks that were built without them. */
int p3d_set_attention_mode(p3d_handle* h, int mode);

/* The training loss of p3d_train_step, p3d_backward, p3d_train_step_device and p3d_profile_step; every one is a SUM over
 * the batch's elements, so with world_size > 1 the summed gradients are the global batch's.
 *   P3D_LOSS_SMOOTH_L1  (default) Smooth-L1, sigma 1 (utils/network.py:49-62, train.py:159): the reference's loss;
 *   P3D_LOSS_BCE        sigmoid cross-entropy on the head's logits, -sum[y log p + (1-y) log(1-p)] with p = sigmoid(logits),
 *                       computed as max(z,0) - z y + log1p(exp(-|z|)) (tf.nn.sigmoid_cross_entropy_with_logits); no
 *                       reference counterpart (BASELINE.json configs[2]).  On the heads without a sigmoid (concat and the
 *                       GroupNorm nets) the raw output is taken as the logits, the only meaning the loss can have there;
 *   P3D_LOSS_L1         L1 sum |pred - y| (the reference's commented-out alternative, train.py:160).
 *   P3D_LOSS_KLD_CC     per-map saliency loss, sum over the B*T maps (one [H, W] frame of one clip each) of
 *                       w_kld KL_m + w_cc (1 - CC_m) (weights: p3d_set_loss_weights, default 1 and 1).  With s the predicted
 *                       saliency, p = s / sum s and q = y / sum y (each left as it is when its sum is 0, the reference's
 *                       `if map.any()`): KL_m = sum q log(eps + q / (p + eps)), eps 2.2204e-16 (utils/metrics.py:338-361, the
 *                       sum of its `score`), and CC_m the Pearson correlation of s and y (utils/metrics.py:227-250) from
 *                       centred sums; a map whose s or y is constant has no CC and adds 0 to the CC term and its gradient.
 *                       Statistics and gradients are float64 on the float32 maps (the reference's KLdiv is float32).  s is
 *                       the stored pred on the sigmoid heads; on the heads without a sigmoid (concat and the GroupNorm nets)
 *                       the raw output is read through a sigmoid, s = 1/(1+exp(-z)), as P3D_LOSS_BCE takes it as logits.
 *   P3D_LOSS_SALIENCY   the per-map loss with the two remaining differentiable metrics and a fixation map f as a third input
 *                       (p3d_upload_fixations; one byte per element, fixated <=> byte >= 128, the /255. > 0.5 of
 *                       p3d_eval_last_frames): sum over the maps of
 *                         w_kld KL_m + w_cc (1 - CC_m) + w_nss (-NSS_m) + w_sim (1 - SIM_m)
 *                       (weights: p3d_set_saliency_weights, default 1, 1, 1, 0; p3d_set_loss_weights does not touch them).
 *                       KL_m, CC_m and s are those of P3D_LOSS_KLD_CC.  With sbar = S/N, A = sum (s - sbar)^2, F the fixated
 *                       count and S_f the sum of s over the fixated elements, NSS_m = (S_f/F - sbar) / sqrt(A/N)
 *                       (utils/metrics.py:200-224, numpy's population std), undefined when F = 0 or A = 0.  With
 *                       u = (s - min s) / (max s - min s), p' = u / sum u and q' likewise from y, SIM_m = sum min(p', q')
 *                       (utils/metrics.py:258-287), undefined when s or y is constant; its gradient holds min s and max s
 *                       fixed, dSIM/ds_i = ([p'_i < q'_i] - sum_j [p'_j < q'_j] p'_j) / sum_j (s_j - min s), the exact one
 *                       touching only the arg-min / arg-max elements and being ambiguous under ties.  An undefined term adds 0
 *                       to the map's loss and gradient, as CC does.  float64 on the float32 maps.  With w_nss = w_sim = 0 the
 *                       loss and the gradients are those of P3D_LOSS_KLD_CC under w_kld, w_cc, bit for bit.
 * Any other kind, or a null handle: -1.  Drops a captured step graph; the next step captures anew.  The first selection of
 * P3D_LOSS_SALIENCY allocates its per-map scratch. */
enum { P3D_LOSS_SMOOTH_L1 = 0, P3D_LOSS_BCE = 1, P3D_LOSS_L1 = 2 };
enum { P3D_LOSS_KLD_CC = 3 };
enum { P3D_LOSS_SALIENCY = 4 };
int p3d_set_loss(p3d_handle* h, int kind);
/* The weights of P3D_LOSS_KLD_CC (default 1, 1): finite, not negative, not both 0; else -1.  They reach the kernels as launch
 * arguments: a change drops a captured step graph. */
int p3d_set_loss_weights(p3d_handle* h, float kld_weight, float cc_weight);
/* The weights of P3D_LOSS_SALIENCY (default 1, 1, 1, 0): each finite and not negative, not all four 0; else -1 and nothing
 * changes.  Launch arguments: a change drops a captured step graph.  Independent of p3d_set_loss_weights. */
int p3d_set_saliency_weights(p3d_handle* h, float kld, float cc, float nss, float sim);
/* The fixation maps of the batch for P3D_LOSS_SALIENCY: fix [B,T,H,W] bytes, copied into a device buffer the handle owns
 * (allocated by the first call; its address then stays, so captured steps remain valid).  Synchronises.
 * While the kind is P3D_LOSS_SALIENCY and w_nss > 0:
 *   p3d_train_step and p3d_backward, which bring x and y from the host, need an upload since the previous such call and
 *     return -1 (p3d_last_error names this function) without one: a stale map must not train silently.  Under
 *     p3d_set_grad_accum that is one upload per micro-batch;
 *   p3d_train_step_device, p3d_profile_step and p3d_debug_schedule reuse the buffer as they reuse x and y, and return -1 only
 *     if nothing was ever uploaded.
 * With w_nss = 0 fixations are neither needed nor read. */
int p3d_upload_fixations(p3d_handle* h, const unsigned char* fix);
/* What a trainer logs under P3D_LOSS_SALIENCY: over this rank's maps of the last step or backward, sums = sum KL_m, sum CC_m,
 * sum NSS_m, sum SIM_m over the maps where each is defined (in map order, in double) and counts = how many those were (NSS is
 * undefined everywhere while w_nss = 0: the fixations are not read).  Under p3d_set_grad_accum: the last micro-batch's.
 * Synchronises.  -1 unless the last step or backward ran P3D_LOSS_SALIENCY. */
int p3d_last_loss_terms(p3d_handle* h, double sums[4], int64_t counts[4]);

/* Regularisation terms added to the loss of p3d_train_step, p3d_backward, p3d_train_step_device and p3d_profile_step: the two
 * collections the reference builds and leaves out of its loss (train.py:161, gn/train_p3d_gn_dataset.py:188-189), as opt-in.
 *   P3D_REG_WEIGHT_DECAY  wd_loss = (1/K) sum_k wd * 0.5 * sum(w_k^2) over the K kernels get_conv_weight makes with wd != 0
 *                         (firstconv1 and the bottleneck kernels; p3d.py:10-16, gn/p3d_gn.py:54-60);
 *   P3D_REG_L2            l2_loss = (1/K2) sum_j l2 * 0.5 * sum(w_j^2) over the kernel_regularizer kernels of scope P3D (the
 *                         decoder-block GN head's layer kernels and P3D/results/kernel; gn/p3d_gn.py:11-21,538).  A net
 *                         without any: -1, nothing changes.
 * terms is a bitmask of the two (0: off, the default).  A scale <= 0 selects the reference's: wd 0.001 on the BatchNorm nets,
 * 0.0005 on the GroupNorm nets; l2 0.0005.  Each variable's coefficient wd/K (l2/K2) is formed in double and rounded to float32
 * once.  The gradient c*w is added to the variable's gradient after its all-reduce, identically on every rank, and the term
 * is taken on the parameters before the step's update.  Each rank's loss is its data loss plus the whole term
 * (p3d_last_regularization gives the term alone).  Drops a captured step graph. */
enum { P3D_REG_WEIGHT_DECAY = 1, P3D_REG_L2 = 2 };
int p3d_set_regularization(p3d_handle* h, int terms, float wd, float l2);
/* The regularisation term of the last step or backward, in double (0 when off). */
int p3d_last_regularization(p3d_handle* h, double* term);
/* The float32 coefficients c the library applies to the trainable variable `name` under the current settings (0 for a term
 * that is off or that does not cover the variable): its gradient gains (c_wd + c_l2) * w. */
int p3d_param_regularization(p3d_handle* h, const char* name, float* c_wd, float* c_l2);

/* tf.train.AdamOptimizer(lr, beta1, beta2, epsilon) (train.py:168; defaults 1e-4, .9, .999, 1e-8). */
int p3d_set_adam(p3d_handle* h, float lr, float beta1, float beta2, float eps);

/* The optimiser of the train step: tf.train.AdamOptimizer (P3D_OPT_ADAM, the default), tf.train.MomentumOptimizer(lr, momentum,
 * use_nesterov) (P3D_OPT_MOMENTUM) or tf.train.GradientDescentOptimizer(lr) (P3D_OPT_SGD).  The reference documents --pretrain
 * as "finetune using SGD" (train.py:27) and its GroupNorm trainer names Momentum (gn/train_p3d_gn_dataset.py:61).
 *   Momentum  accum = accum * momentum + g; var -= lr * accum, or with use_nesterov var -= g * lr + accum * momentum * lr
 *             on the updated accum (TF's ApplyMomentum); SGD var -= lr * g (ApplyGradientDescent).  Float32, every product
 *             and sum rounded on its own (no fused multiply-add).
 * Switching kind gives a fresh optimiser: its slots and step count are zeroed, as a newly built TF optimiser has them.  The same
 * kind with new hyper-parameters keeps the state.  P3D_OPT_ADAM takes lr and keeps beta1, beta2, epsilon from p3d_set_adam
 * (which is unchanged).  The optimiser still runs as two parts after their all-reduces, and a regularisation term fuses into
 * it as it does into Adam.  Returns -1 for an unknown kind, a non-finite lr or momentum, or a negative momentum.
 * p3d_init_params zeroes the slots and the step count of every kind. */
enum { P3D_OPT_ADAM = 0, P3D_OPT_MOMENTUM = 1, P3D_OPT_SGD = 2 };
int p3d_set_optimizer(p3d_handle* h, int kind, float lr, float momentum, int use_nesterov);
/* Optimiser slots of the trainable variable `var`, count = its element count: Adam slot 0 is m (TF's <var>/Adam), slot 1 is
 * v (<var>/Adam_1); Momentum slot 0 is the accumulator (<var>/Momentum); SGD has none.  -1 for a slot the current kind
 * lacks, a non-trainable or unknown variable, or a wrong count. */
int p3d_get_slot(p3d_handle* h, const char* var, int slot, float* host, int64_t count);
int p3d_set_slot(p3d_handle* h, const char* var, int slot, const float* host, int64_t count);
/* Completed optimiser steps t (every kind); Adam's next step uses the bias correction of step t + 1.  Setting needs t >= 0. */
int p3d_get_optimizer_step(p3d_handle* h, int64_t* t);
int p3d_set_optimizer_step(p3d_handle* h, int64_t t);

/* Gradient clipping by the global norm, as tf.clip_by_global_norm does it ahead of apply_gradients (an addition: the reference
 * trains with Adam alone, which does not see the gradient's scale; its loss is a SUM over every output element, so Momentum
 * and SGD see a gradient that grows with the batch and the clip size).  clip_norm = 0: off, the default; > 0: on; +inf:
 * measure only; negative or NaN: -1.  With the option on, every train step computes, after the all-reduces and before any
 * optimiser launch,
 *   sumsq = sum g'^2 over every element of every trainable variable, g' the gradient the optimiser is about to apply (with a
 *           regularisation term on, g' = fadd(g, fmul(c, w)) in float32); each square exact in double, the sum in double in a
 *           fixed order (the same bits on every run, however the step cuts the range into launches);
 *   norm  = sqrt(sumsq) in double;
 *   scale = (float)(clip_norm / max(norm, (double)clip_norm)): exactly 1.0f while norm <= clip_norm; 1.0f under +inf; NaN when
 *           norm is NaN or inf (the step then poisons the weights as the unclipped step would).
 * The optimiser's update then runs on fmul(g', scale), rounded once, and is otherwise the chosen optimiser's arithmetic: a
 * threshold that is not reached gives the bits of the unclipped step.  The gradient buffer is not rewritten: p3d_get_grad
 * returns what it returns without clipping.  The first optimiser part no longer overlaps the stem's filter gradient (no update
 * may start before the norm is known); that slot takes the first range of the sum instead.  p3d_backward computes the three
 * values and scales nothing.  Drops a captured step graph.
 * p3d_get_grad_norm: the values of the last train step or p3d_backward (any pointer may be NULL); -1 while the option is off or
 * before the first step or backward since it was set.  Under data parallelism the norm is taken after the all-reduce, so every
 * rank computes the same scale. */
int p3d_set_grad_clip(p3d_handle* h, float clip_norm);
int p3d_get_grad_norm(p3d_handle* h, double* sumsq, double* norm, float* scale);

/* Exponential moving average of the weights, as tf.train.ExponentialMovingAverage(decay[, num_updates]).apply(
 * tf.trainable_variables()) run after the train op (an addition: the reference scores single checkpoints).  Off by default; off,
 * a step launches what it launched before the option existed.  decay < 0 (e.g. -1): off; finite with 0 <= decay < 1: on;
 * anything else (1, above 1, NaN, +inf): -1, nothing changed.  A shadow s exists for every TRAINABLE variable -- BatchNorm's
 * moving statistics have none.  After the optimiser has updated p in a train step (p3d_backward never touches the shadows),
 *   s = s - (s - p) * om        float32, every operation rounded on its own, no fused multiply-add
 * (TF's assign_moving_average).  om:
 *   warmup == 0   om = (float)(1.0 - decay): the subtraction in double, rounded once, as TF does with a Python float -- which is
 *                 why decay is a double here: (float)(1.0 - 0.999) is not 1.f - 0.999f.
 *   warmup != 0   TF's num_updates: t = (float)steps, steps = the completed optimiser steps including this one (what
 *                 p3d_get_optimizer_step returns after the step); q = (1.f + t) / (10.f + t); d = fminf((float)decay, q);
 *                 om = 1.f - d, all in float32.
 * No TensorFlow was available to pin this against: the text above is the contract, and tests/ema_ref.py replays it bit for bit.
 * The shadows (one float per trainable element, allocated the first time the option is switched on) are seeded with a copy of
 * the parameters whenever the option goes from off to on, as TF initialises a shadow from its variable, and again by
 * p3d_init_params while it is on.  A new decay or warm-up flag while on, p3d_set_optimizer and p3d_set_param leave them alone.
 * Each optimiser launch of the step is followed by one launch of ema_kernel over the same range.  Under data parallelism every
 * rank holds the same weights after the update, hence the same shadows; nothing is communicated.  Drops a captured step graph.
 * p3d_get_ema / p3d_set_ema_var: the shadow of `var`; -1 while the option is off, for an unknown or non-trainable variable, or
 * a wrong count.
 * p3d_ema_swap exchanges parameters and shadows of every trainable, bit for bit, in one launch, so that p3d_forward,
 * p3d_predict_windows, p3d_eval_last_frames and p3d_pred_maps_u8 score the averaged weights without a second network; a second
 * call restores both (-1 while the option is off).  p3d_ema_swapped: 1 while exchanged, else 0.  While exchanged
 * p3d_train_step*, p3d_backward, p3d_profile_step, p3d_set_param, p3d_init_params and p3d_set_ema return -1 (a forgotten swap
 * must not average the averages), and p3d_get_param returns what the parameter buffer then holds -- the shadows -- while
 * p3d_get_ema returns the parameters. */
int p3d_set_ema(p3d_handle* h, double decay, int warmup);
int p3d_get_ema(p3d_handle* h, const char* var, float* host, int64_t count);
int p3d_set_ema_var(p3d_handle* h, const char* var, const float* host, int64_t count);
int p3d_ema_swap(p3d_handle* h);
int p3d_ema_swapped(p3d_handle* h);

/* Gradient accumulation over micro-batches: the TF-1 idiom of running the gradients K times into accumulators and calling
 * apply_gradients once (an addition: the reference applies every batch of 2, train.py:39; with BatchNorm on batch statistics in
 * the whole backbone a larger batch changes what is normalised, and accumulation is how the effective batch grows without that).
 * k = 1: off, the default -- a step launches what it launched before the option existed and no memory is allocated; k >= 2: on;
 * k < 1: -1, nothing changed.  With k >= 2 every call of p3d_train_step, p3d_train_step_device, p3d_profile_step or
 * p3d_debug_schedule is one MICRO-STEP j = pending of a cycle of k:
 *   j < k-1   accumulates.  Forward with training on and the moving-statistics updates, loss, backward.  No all-reduce, no
 *             optimiser, norm or moving-average launch; the optimiser's step count does not move, weights and slots keep their
 *             bits.  Then acc = g (j = 0: a copy of the bits, -0 stays -0) or acc = fadd(acc, g) (j > 0) in float32 over every
 *             trainable element.  The returned loss is this micro-batch's data loss alone and p3d_last_regularization gives 0;
 *             p3d_get_grad returns this micro-batch's gradient; p3d_get_grad_norm keeps the values of the last update.
 *   j = k-1   applies.  After the backward the gradient buffer becomes fadd(acc, g), and everything downstream runs on it as on
 *             any gradient, in the usual order: the all-reduce (the sum over ranks of each rank's accumulated sum), the
 *             regularisation term g + c*w (once per update), the global norm and its scale, the optimiser of the current kind in
 *             its two parts, the moving average, the step count + 1.  pending returns to 0.  p3d_get_grad returns the
 *             accumulated (and reduced) gradient; the loss is this micro-batch's data loss plus the regularisation term.
 * Gradients are SUMMED, not averaged: every loss here is a sum over the batch, and data parallelism sums in the same way, so k
 * micro-batches of B clips give the gradient of one batch of k*B clips (up to BatchNorm's statistics, which stay per
 * micro-batch).  Adam does not see the scale; with Momentum or SGD scale lr by 1/k, or clip.  The order is fixed,
 * ((g0 + g1) + g2) + ... per element with each sum rounded once to float32: the same bits on every run.
 * The accumulator holds one float per trainable element and is allocated the first time k >= 2 is set.  Any call of
 * p3d_set_grad_accum (with the same k too) and p3d_init_params discard a partial sum and set pending to 0; p3d_set_param,
 * p3d_set_optimizer, p3d_set_ema, p3d_ema_swap and p3d_backward leave it alone -- p3d_backward stays the parity hook and neither
 * reads nor writes the accumulator.  While k >= 2 a captured step (P3D_GRAPH=1) is not used: a cycle has three launch lists, and
 * the step runs the eager one; the call drops a captured step graph.  Checkpoints do not store a partial sum: save at update
 * boundaries (pending = 0).
 * p3d_get_grad_accum: k, and pending = the micro-steps accumulated since the last update, 0 .. k-1 (either pointer may be NULL). */
int p3d_set_grad_accum(p3d_handle* h, int k);
int p3d_get_grad_accum(p3d_handle* h, int* k, int* pending);

/* Clip augmentation on the device (an addition: the reference's loader only resizes, dataflow.py:187-191, and its clips overlap in
 * 15 of 16 frames).  Off by default; off, p3d_train_step issues what it issued before the option existed.  The transform acts on
 * the three staged inputs of a train step -- x [B,T,H,W,3], y [B,T,H,W] and, when the loss reads them (P3D_LOSS_SALIENCY with
 * w_nss > 0), the fixation bytes [B,T,H,W] -- with ONE set of decisions per clip applied alike to all three, so the maps stay
 * registered to the frames.  Per clip, in this order:
 *   1 crop and resize back: the window [y0, y0 + ch) x [x0, x0 + cw) of every frame of x (each channel on its own) and of y is
 *     resized to H x W by the float32 cv2.INTER_LINEAR law of p3d_resize_linear (same coordinates, float32 weights, horizontal
 *     pass then vertical, no fused multiply-add).  A fixation cell (h, w) becomes 255 if some byte >= 128 at (r, c) inside the
 *     window has (r - y0) * H / ch == h and (c - x0) * W / cw == w (integer division), else 0.  A window equal to the whole frame
 *     is a copy of the bits, of the fixation bytes as well: no arithmetic, NaN, inf and -0 pass through;
 *   2 horizontal flip, w -> W - 1 - w;   3 temporal reversal, t -> T - 1 - t;   both on x, y and the fixations;
 *   4 photometric, x only: x' = fadd(fmul(x, a), b) in float32, each operation rounded on its own; a == 1 and b == 0 is a copy
 *     of the bits.
 * 1-3 are one gather; every element is written once.  The decisions are drawn on the host from the step's seed and the clip's
 * GLOBAL index g = rank * B + b, so a run can be replayed and data-parallel ranks draw differently: draw j = 0..6 is
 *   z = seed ^ 0xA5A5A5A5A5A5A5A5;  z += 0x9E3779B97F4A7C15 * (1 + 8 g + j)   (mod 2^64);
 *   z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;  z ^= z >> 31   (SplitMix64's finaliser);
 *   u = (z >> 11) * 2^-53 in double, and
 *   j = 0  flip if u < p_flip;                  j = 1  reverse if u < p_reverse;
 *   j = 2  s = 1 - u (1 - min_scale); ch = clamp(floor(s H + 0.5), 1, H); cw = clamp(floor(s W + 0.5), 1, W);
 *   j = 3  y0 = floor(u (H - ch + 1));          j = 4  x0 = floor(u (W - cw + 1));
 *   j = 5  a = (float)(1 + (2u - 1) contrast);  j = 6  b = (float)((2u - 1) brightness)
 * in double on the float32 settings.  tests/augment_ref.py replays transform and draws bit for bit.
 * p3d_set_augment: NULL or the neutral values (0, 0, 1, 0, 0) switch the option off.  Probabilities in [0, 1], 0 < min_scale <= 1,
 * 0 <= contrast < 1, brightness >= 0, all finite; anything else: -1, nothing changes.  The first switch-on allocates the scratch
 * (a copy each of x, y and the fixations, and the decision table).  The scratch is private and the staged buffers do not move: a
 * captured step graph stays valid.
 * While on, p3d_train_step -- the one entry point that takes host inputs and trains -- augments with its own `seed` after it has
 * brought x and y from the host and before the forward pass; under p3d_set_grad_accum every micro-step is such a call.  The
 * fixations are transformed exactly when the loss will read them; p3d_train_step already demands a fresh upload for each call
 * then, so no buffer is transformed twice.  The launches run ahead of the step, outside its launch list and outside a captured
 * step.  NEVER augmented: p3d_backward (the parity hook), p3d_forward*, p3d_predict_windows, the evaluation entry points,
 * p3d_train_step_device, p3d_profile_step, p3d_debug_schedule.
 * p3d_augment_inputs is the explicit form for the device-resident path: it transforms what p3d_upload_inputs (and
 * p3d_upload_fixations, when the loss reads them) staged, in place through the scratch, once per call; p3d_augment_inputs and then
 * p3d_train_step_device is p3d_train_step for the same seed.  Synchronises.
 * p3d_last_augment: the decisions of the last augmentation, geom [B][6] = flip, reverse, y0, x0, ch, cw and photo [B][2] = a, b
 * (either may be NULL).  p3d_last_augment_ms: the HIP-event time of its launches (synchronises).  While the option is off, and
 * before the first augmentation since it was switched on, the three return -1.  p3d_get_augment: the settings (neutral while
 * off) and whether the option is on; either pointer may be NULL.  Checkpoints store nothing of this. */
typedef struct p3d_augment { float p_flip, p_reverse, min_scale, contrast, brightness; } p3d_augment;
int p3d_set_augment(p3d_handle* h, const p3d_augment* cfg);
int p3d_get_augment(p3d_handle* h, p3d_augment* cfg, int* on);
int p3d_augment_inputs(p3d_handle* h, uint64_t seed);
int p3d_last_augment(p3d_handle* h, int32_t* geom, float* photo);
int p3d_last_augment_ms(p3d_handle* h, double* ms);

/* ---- intermediate tensors (tf fetches of graph tensors; parity/debug taps).  Names:
 *      conv1_custom, conv1_custom_bn_relu, pool1..pool4, block<i>/conv1_bn_relu, block<i>/st,
 *      block<i>/out, deconv3_re, deconv4_conv1, logits, pred. */
int p3d_activation_info(p3d_handle* h, const char* name, int64_t shape[5]);
int p3d_get_activation(p3d_handle* h, const char* name, float* host, int64_t count);

/* ---- schedule of one train step (TEST HOOK, tests/test_gpu_schedule.py): runs p3d_train_step_device once and writes every stream
 *      operation it issued, in host issue order, one per line: "L <stream> <kernel> [@op]" (launch), "M <stream> <what>" (async
 *      fill), "R <stream> e<k>" (event record), "W <stream> e<k>" (stream waits for event), "C <stream> allreduce <lo> <hi>".
 *      Under p3d_set_grad_accum, "G <stream> store|add|finish <lo> <hi>" ahead of a launch of the accumulator is a note, not a
 *      stream operation.  A side-stream job that the walk parked until it reached the encoder carries the tag of the op that
 *      released it, not of the op whose backward queued it.
 *      Streams: main, side (filter gradients), comm (all-reduce).  `needed` receives the size of the text; call with a buffer
 *      at least that large (a first call with text = NULL runs the step, too).  Synchronises. */
int p3d_debug_schedule(p3d_handle* h, float dropout_rate, uint64_t seed, char* text, int64_t cap, int64_t* needed);

/* ---- schedule perturbation (TEST HOOK, tests/test_gpu_stream_hazards.py): the step is bit-reproducible, so a correct schedule gives
 *      the same bits however its three streams drift against each other.
 *      mode 0: off.  1: serial -- the issuing stream is synchronised after every launch / fill / all-reduce (host issue order).
 *      2: slow -- a bounded delay kernel of delay_us goes onto `stream` (0 main, 1 side, 2 comm) ahead of every launch, fill and
 *      all-reduce issued on it.  Stays until changed, for the calls the calling thread makes; only this handle's streams are
 *      touched.  Refused (-1) when P3D_GRAPH is set, as p3d_debug_schedule is; ignored in dry and profiling passes.  delay_us in
 *      [1, 2000].  The delay kernel is one block whose lane 0 polls the 100 MHz wall clock between sleeps and leaves when the time
 *      is up or after a fixed number of polls (about 10x the delay); it reads and writes no memory and is not part of the
 *      p3d_debug_schedule trace.
 *      p3d_debug_perturb_count: the delay kernels and synchronisations inserted since the last call to p3d_debug_perturb.
 *      p3d_debug_perturb_selftest shows that the hook can see a missing wait.  Two pooled streams A and B, two buffers of 4096
 *      floats: buf = 1.0 (complete); on A a launch overwrites buf with 2.0 and an event is recorded; B waits for it only if
 *      with_wait; on B a launch copies buf to out[4096]; both are synchronised.  All through the launch / event funnel of the
 *      step, under `mode` (2: `slow` 0 holds back A, the producer's stream, 1 holds back B, the consumer's).  Every value read
 *      is a valid float in allocated memory. */
int p3d_debug_perturb(p3d_handle* h, int mode, int stream, int delay_us);
int p3d_debug_perturb_count(p3d_handle* h, int64_t* delays, int64_t* syncs);
int p3d_debug_perturb_selftest(int device, int mode, int slow, int delay_us, int with_wait, float* out);

/* ---- what the host layer holds outside the graph's arenas (TEST HOOK, tests/test_gpu_private_resources.py): the device blocks
 *      and bytes, and the timing events, that are live in this process at the moment of the call -- the stores of an open video,
 *      training set, prior or fixation pool, the baseline of p3d_set_eval_extra, the buffers of an op-level entry point while it
 *      runs.  Process-wide over all handles; a handle's arenas, its streams and its ordering events are not counted.  A facility
 *      that is closed, and a handle that is destroyed, return what they took.  Any pointer may be NULL. */
int p3d_debug_private_resources(int64_t* blocks, int64_t* bytes, int64_t* events);

/* ---- decisions of the last forward (TEST HOOK, tests/test_gpu_pinned.py): the ReLU gates and max-pool choices the backward pass of
 *      this handle will use -- so that the oracle can differentiate the SAME piecewise-linear branch (a float32 forward takes
 *      a handful of near-zero decisions differently from a float64 one, and each moves a gradient tensor by per cent).
 *      Site `index` (0 .. count-1, graph order) is a normalise / ReLU pass ("bn": out1 / out2 are NON-ZERO where the gate of the
 *      first / second BatchNorm branch -- TF scopes name1 / name2, name2 empty when there is one -- is open; produced by the
 *      pass's own backward kernel on a gradient of ones with the statistics terms off) or a max-pool ("pool": out1 is the pool's
 *      input as this handle holds it; its arg-max follows from it exactly).  count = elements of `shape`.  Call after a forward
 *      or backward pass of the whole graph with BatchNorm fusion off; synchronises. */
int p3d_debug_decision_count(p3d_handle* h);
int p3d_debug_decision_info(p3d_handle* h, int index, const char** kind, const char** name1, const char** name2, int64_t shape[5]);
int p3d_debug_decision_get(p3d_handle* h, int index, float* out1, float* out2, int64_t count);

/* ---- one bottleneck in isolation (BASELINE.json configs[0], SURVEY.md 8d cfg 1 "standalone variant"): the forward of
 *      Bottleneck(...).infer() (p3d.py:83-136; gn/p3d_gn.py:127-179 for the GN structures) number `block_id`
 *      (0 .. sum(blocks)-1) of this handle's graph on a caller-supplied input, with the handle's current parameters.
 *      Shapes are those the block has inside the graph (p3d_block_info).  BatchNorm uses batch statistics, as
 *      everywhere in the backbone. */
int p3d_block_info(p3d_handle* h, int block_id, int64_t in_shape[5], int64_t out_shape[5]);
int p3d_block_forward(p3d_handle* h, int block_id, const float* in, int64_t in_count, float* out, int64_t out_count);
/* The same bottleneck, forward then backward: `dout` is the gradient of its output, `din` receives the gradient of its input; the
 * gradients of the block's own variables are read with p3d_get_grad afterwards (every other variable's gradient reads 0).
 * Parity hook for gradients at sizes where the whole graph is out of the oracle's reach. */
int p3d_block_backward(p3d_handle* h, int block_id, const float* in, int64_t in_count, const float* dout, int64_t out_count, float* din);

/* ---- device-resident stepping for measurement: inputs already in HBM (bench.py).
 *      p3d_device_inputs returns the handle's own x / y staging buffers (device pointers,
 *      [B,T,H,W,3] and [B,T,H,W] floats); fill them once with p3d_upload_inputs, then call
 *      p3d_train_step_device / p3d_forward_device repeatedly; p3d_synchronize drains the stream. */
int p3d_upload_inputs(p3d_handle* h, const float* x, const float* y);
int p3d_train_step_device(p3d_handle* h, float dropout_rate, uint64_t seed);
int p3d_forward_device(p3d_handle* h, int training, float dropout_rate, uint64_t seed);
int p3d_last_loss(p3d_handle* h, float* loss);          /* synchronises */
int p3d_synchronize(p3d_handle* h);

/* ---- per-launch timing of one train step with HIP events on the stream the kernels are launched
 *      on (the data behind bench.py's roofline object).  One record per kernel launch, in launch
 *      order.  Writes up to `cap` records; returns the number of launches. */
typedef struct p3d_op_time {
    char name[64];        /* graph op the launch belongs to (block7/convS, deconv3, ...) */
    char kernel[48];      /* kernel symbol (igemm_kernel<128,128>, bn_apply_kernel<1>, ...) */
    double ms;            /* HIP-event duration of this launch */
    double flops;         /* algorithmic FLOPs of this launch (2*MACs) */
    double bytes;         /* algorithmic HBM bytes of this launch (operands read once, result written once) */
    int phase;            /* 0 forward, 1 backward, 2 optimiser */
} p3d_op_time;
int p3d_profile_step(p3d_handle* h, float dropout_rate, uint64_t seed, p3d_op_time* out, int cap);

/* ---- data parallel (no reference counterpart: the reference is single-device, train.py:73).
 *      Rank 0 creates an id, every rank passes the same bytes to p3d_comm_init. */
#define P3D_COMM_ID_BYTES 128
int p3d_comm_unique_id(void* id_out);
int p3d_comm_init(p3d_handle* h, const void* id);
/* GPUs this process can see (hipGetDeviceCount), -1 on error.  A launcher may give every rank ALL the node's GPUs (torch.distributed.run:
 * rank r uses device LOCAL_RANK) or exactly one (per-rank HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES: every rank uses device 0);
 * bench.py asks before it picks p3d_config.device. */
int p3d_device_count(void);
/* What RCCL itself says about the handle's communicator (ncclCommCount / ncclCommUserRank / ncclCommCuDevice): *n_ranks = 0 when the
 * handle has none.  bench.py prints it as "rccl_ranks" at N > 1 and refuses a run where it differs from --gpus, so that a scaling
 * line cannot come from ranks that never met. */
int p3d_comm_info(p3d_handle* h, int* n_ranks, int* rank, int* device);
/* Audit of the bucketed gradient hand-over (test hook; needs no communicator).  Runs forward + loss + backward with
 * buckets of `bucket_floats` and, at every point where a bucket [lo, hi) of the flat gradient buffer would be handed to
 * the all-reduce, waits for the work queued so far and copies the range out instead.  Returns the number of buckets
 * (their ranges and the op index after whose backward each was handed over go to lo / hi / after_op, up to `cap`),
 * *n_train = floats in the flat buffer, *stale = how many bucket elements differed from the final gradient, i.e.
 * were handed over before their last producer had run (must be 0). */
int p3d_debug_bucket_audit(p3d_handle* h, float dropout_rate, uint64_t seed, int64_t bucket_floats, int64_t* lo, int64_t* hi,
                           int32_t* after_op, int cap, int64_t* n_train, int64_t* stale);

/* Test hook: synchronises the device and returns how many arrival counters of the K-slice exchange scratch are non-zero
 * (every sliced launch re-zeroes its own: anything but 0 means a launch left the scratch dirty); -1 on a HIP error. */
int64_t p3d_debug_dirty_counters(void);

/* Test hook (process-wide): on SIGABRT / SIGSEGV print a C-level backtrace to stderr before dying, and the message of an uncaught
 * C++ exception (tests/conftest.py installs it: Python's faulthandler shows Python frames only). */
int p3d_debug_install_abort_trace(void);

/* Test hook (process-wide): force the tile / K-slice plan of the convolution kernels where a problem allows it, so that
 * every instantiation is reachable from the op-level parity tests.  igemm_tile: 0 = 64x64, 1 = 128x64, 2 = 128x128,
 * -1 = the plan's choice; igemm_splits: K-slices, 0 = the plan's; wgrad_tm / wgrad_tn: 64 or 128, 0 = the plan's. */
int p3d_debug_force_plan(int igemm_tile, int igemm_splits, int wgrad_tm, int wgrad_tn);

/* ---- single operators on host arrays (the TF ops the path is made of), for op-level parity
 *      tests.  SAME padding, NDHWC, filters [kd,kh,kw,Cin,Cout]; strides s[3] = (sd,sh,sw). */
int p3d_op_conv3d(int device, const float* x, const int64_t xshape[5], const float* w, const int64_t wshape[5],
                  const int s[3], const float* bias, float* y);                       /* tf.nn.conv3d (+bias_add) */
int p3d_op_conv3d_backprop_input(int device, const float* dy, const float* w, const int64_t wshape[5],
                                 const int s[3], const int64_t xshape[5], float* dx);
int p3d_op_conv3d_backprop_filter(int device, const float* x, const int64_t xshape[5], const float* dy,
                                  const int64_t wshape[5], const int s[3], float* dw, float* dbias);
/* tf.layers.conv3d_transpose 'same'; kernel [kd,kh,kw,Cout,Cin] */
int p3d_op_conv3d_transpose(int device, const float* x, const int64_t xshape[5], const float* k,
                            const int64_t kshape[5], const int s[3], const float* bias, float* y);
/* Test hook: the stem's filter gradient through its BatchNorm + ReLU (tf.gradients of p3d.py:172-174 w.r.t. firstconv1), once with
 * the normalisation's backward evaluated on the kernel's operand (what the train step runs) and once as two launches.  x [N,D,H,W,3];
 * y, dz [N,D,ceil(H/2),ceil(W/2),64]; tab [5][64] = scale, shift, mean, invstd, gamma; coef [64][2]; both results [1,7,7,3,64]. */
int p3d_debug_stem_wgrad_through_bn(int device, const float* x, const int64_t xshape[5], const float* y, const float* dz, const float* tab,
                                    const float* coef, int batch, float* dw_fused, float* dw_two_launches);
/* Test hooks: BatchNorm statistics behind a conv (tf.layers.conv3d / conv3d_transpose, then tf.layers.batch_normalization
 * in training).  Shapes as p3d_op_conv3d (transpose = 0) or p3d_op_conv3d_transpose (transpose = 1).
 * p3d_debug_conv_bn_stats: the conv's launches with the statistics epilogue, sized and routed like the network's, then the
 * finalize (batch statistics, momentum-0.99 update of the moving statistics, eps 1e-3, gamma 1, beta 0).  w2 non-null: a sibling
 * pair of forward convs on one input (ST_B), y2 its second output.  moving [pairs][2][C] = (mean, variance), updated in place;
 * stats [pairs][4][C] = scale, shift, mean, invstd; nparts[pairs] = epilogue partials written (0: the small-tensor BatchNorm
 * takes the tensor and computes its own -- the hook's statistics then come from p3d_bn_stats, not from bn_small.hip, whose
 * statistics p3d_debug_bn_pass covers); *kernel = the plan of the first launch.
 * p3d_debug_stat_parts (host only, no HIP call): the partials such a conv writes and the room the network reserves for them.
 * p3d_debug_igemm_groupable (host only): would two sibling forward convs of this shape go out as one grouped launch (1 / 0). */
int p3d_debug_conv_bn_stats(int device, const float* x, const int64_t xshape[5], const float* w, const float* w2, const int64_t wshape[5],
                            const int s[3], const float* bias, int transpose, float* moving, float* y, float* y2, float* stats,
                            int* nparts, const char** kernel);
/* Test hook: one BatchNorm normalise / ReLU / add pass (modes of bn_apply: 0 relu(bn1(y1)), 1 relu(bn1(y1) + r),
 * 2 relu(bn1(y1) + bn2(y2)), 3 relu(bn1(y1)) + relu(bn2(y2)), 4 r + relu(bn1(y1))) on M rows of C channels, forward then
 * backward, launched as the network launches it.  The operands are channel slices of wider rows: y1 and dy1 [M][ld1] at column
 * off1, y2 and dy2 [M][ld2] at off2 (y2 is the second BN input or the residual r; null for mode 0), z and dz [M][ldz] at offz;
 * strides and offsets are multiples of 4 with off + C <= ld.  In/out: z, dy1 and dy2 keep what they held outside their C
 * columns; dy2 (modes 1-4) holds the gradient to add to when acc2.  The stand-in statistics (p3d_bn_stats) read the slices too.
 * params [bns][2][C] = gamma, beta; moving [bns][2][C] = moving (mean, variance), updated in place when update_moving and the
 * BN uses batch statistics (batch1 / batch2).  grads [bns][2][C] = dgamma, dbeta.  drop_rate in [0, 1): the pass is a dropout
 * site's (mask as defined at p3d_forward, e = row * C + c, scale 1 / (1 - drop_rate)) keyed by seed -- passed as an argument,
 * or read from device memory when seed_dev; a rate outside [0, 1) is refused.  path: 0 = the network's rule (bn_path: a pass
 * that drops out takes neither the small-tensor kernels nor fold-apply), 1 = small-tensor kernels, 2 = fold-apply, 3 = finalize
 * + apply (the last two with the three-launch backward); a forced path the kernels cannot take -- 1 or 2 with drop_rate > 0
 * among them -- is an error that writes nothing.  info[3] = path taken, forward statistics partials per BN, backward partials. */
int p3d_debug_bn_pass(int device, int mode, int64_t M, int C, const float* y1, int ld1, int off1, const float* y2, int ld2, int off2,
                      const float* params, int batch1, int batch2, int update_moving, const float* dz, int acc2, float drop_rate,
                      uint64_t seed, int seed_dev, int path, float* z, int ldz, int offz, float* dy1, float* dy2, float* grads,
                      float* moving, int* info);
/* Test hook: one GroupNorm normalise / ReLU / add pass of the GN network (modes of gn.hip: 0 relu(gn1(y1)), 1 relu(gn1(y1) + r),
 * 2 relu(gn1(y1) + gn2(y2)) (forward only), 3 relu(gn1(y1)) + relu(gn2(y2)), 4 r + relu(gn1(y1)), 5 gn1(y1),
 * 6 relu(gn1(y1) + r * cs[n,c] * ss[row])) on N samples of R rows of C channels, G groups, forward then backward, launched as
 * the network launches it.  y1 [N*R][ld1]; y2 [N*R][ld2] = the second GN input or the residual r (null for modes 0, 5);
 * z and dz [N*R][ldz]; params [gns][2][C] = gamma, beta; cs [N][C] and ss [N*R] for mode 6.  In/out: z, dy1 [N*R][ld1] and
 * dy2 [N*R][ld2] keep what they held outside the C columns of a row; dy2 (modes 1, 3, 4, 6) holds the gradient to add to when
 * acc2; grads [gns][2][C] = dgamma, dbeta are stored.  drop_rate > 0: dropout on z with the kernels' hash of seed.
 * tables [gns][4][N][C] = scale, shift, mean, invstd.  path: 0 = the network's rule, 1 = the one-launch small-tensor kernels,
 * 2 = statistics / finalize / apply; a forced path the kernels cannot take is an error.  *info = path taken. */
int p3d_debug_gn_pass(int device, int mode, int N, int R, int C, int G, float eps, const float* y1, int ld1, const float* y2, int ld2,
                      int ldz, const float* params, const float* cs, const float* ss, const float* dz, int acc2, float drop_rate,
                      uint64_t seed, int path, float* z, float* dy1, float* dy2, float* grads, float* tables, int* info);
/* Test hook: CBAM forward and backward (the network's cbam(): p3d_cbam_forward / p3d_cbam_backward on a site's scratch layout).
 * x [N*D*H*W][ld]; k0 [C][C/8], b0 [C/8], k1 [C/8][C], b1 [C], k7 [7][7][7][2][1]; chunks = row chunks per sample (0: the
 * network's rule); dout [N*D*H*W][C] = gradient of the CBAM output.  Out: cs [N][C], sp [N*D*H*W][2], ss [N*D*H*W].  In/out:
 * dx [N*D*H*W][ld] (overwritten, or added to when accx), pgrads = dk0 | db0 | dk1 | db1 | dk7 (added to).  *info = chunks used. */
int p3d_debug_cbam(int device, int N, int D, int H, int W, int C, const float* x, int ld, const float* k0, const float* b0,
                   const float* k1, const float* b1, const float* k7, int chunks, const float* dout, int accx, float* cs, float* sp,
                   float* ss, float* dx, float* pgrads, int* info);
/* Test hook: the output head (head() of the network) forward, then both gradients, through the launchers the network calls.
 * transpose 1: tf.layers.conv3d_transpose(x, 1, 3, 2, 'same'), logits / pred / dlogits [N,2D,2H,2W]; 0: the stride-1
 * tf.layers.conv3d(x, 1, 3, 1, 'same') of the GN decoder-block network, [N,D,H,W].  x, dx [N,D,H,W,C]; k [27][C] (the kernel
 * [3,3,3,1,C], or [3,3,3,C,1] at stride 1); bias [1]; sigmoid: pred = sigmoid(logits), else pred = logits.  dk and dbias
 * hold the gradients to add to on entry.  fwd_path: 0 = the network's rule, 1 = L = C/4 lanes per position, 2 = one thread
 * per position; filter_path: 0 = the rule, 1 = four channels per thread with HEAD_FOLD-block groups folded in two levels,
 * 2 = one channel per thread, one-level fold (stride 1: both 0, one kernel each).  A forced kernel the shape does not allow
 * is an error.  info[4] = forward kernel (1 lanes, 2 per position, 3 stride 1) and its blocks, filter-gradient kernel
 * (1 four channels, 2 one channel, 3 stride 1) and its blocks. */
int p3d_debug_head(int device, int transpose, int N, int D, int H, int W, int C, const float* x, const float* k, const float* bias,
                   int sigmoid, const float* dlogits, int fwd_path, int filter_path, float* logits, float* pred, float* dx, float* dk,
                   float* dbias, int* info);
/* Test hook: the Smooth-L1 loss and dL/dlogits (p3d_loss, as the network's loss launches it) on n elements placed
 * `offset` (0-3) elements into the device buffers: offsets 1-3 misalign them and force the scalar path.  through_sigmoid:
 * dlogits = dL/dpred * pred * (1 - pred).  *loss is added to.  info[2] = path taken (1 float4, 2 scalar), blocks. */
int p3d_debug_smooth_l1(int device, const float* pred, const float* target, int64_t n, int through_sigmoid, int offset, double* loss,
                        float* dlogits, int* info);
/* Test hook: the loss of kind (P3D_LOSS_*) and dL/dlogits as the network launches it, on logits, pred (sigmoid(logits) when
 * through_sigmoid, else the logits again) and target placed as p3d_debug_smooth_l1 places them, with its `info`; kind
 * P3D_LOSS_SMOOTH_L1 is p3d_debug_smooth_l1 (logits unused).  *loss is added to. */
int p3d_debug_loss(int device, int kind, const float* logits, const float* pred, const float* target, int64_t n, int through_sigmoid,
                   int offset, double* loss, float* dlogits, int* info);
/* Test hook: P3D_LOSS_KLD_CC as the network launches it (its three launches) on `maps` maps of map_elems elements each,
 * logits, pred and target placed as p3d_debug_loss places them; through_sigmoid: s = pred, else s = sigmoid(logits) (pred
 * unused).  *loss is added to; per_map [maps][2] = KL_m, CC_m (NaN where CC is undefined); dlogits = dL/dlogits.
 * info[3] = launches, blocks per map, path taken (1 float4, 2 scalar). */
int p3d_debug_map_loss(int device, const float* logits, const float* pred, const float* target, int64_t maps, int64_t map_elems,
                       int through_sigmoid, int offset, float kld_weight, float cc_weight, double* loss, float* dlogits,
                       double* per_map, int* info);
/* Test hook: P3D_LOSS_SALIENCY as the network launches it (its three launches), as p3d_debug_map_loss with the fixation bytes
 * fix [maps * map_elems] placed `offset` bytes into their device buffer (may be null when nss_weight is 0: they are not read)
 * and the four weights (finite, not negative).  per_map [maps][4] = KL_m, CC_m, NSS_m, SIM_m (NaN where undefined); info as
 * p3d_debug_map_loss. */
int p3d_debug_saliency_loss(int device, const float* logits, const float* pred, const float* target, const unsigned char* fix,
                            int64_t maps, int64_t map_elems, int through_sigmoid, int offset, float kld_weight, float cc_weight,
                            float nss_weight, float sim_weight, double* loss, float* dlogits, double* per_map, int* info);
/* Test hook: one Adam launch (p3d_opt_step, as the network's optimiser step launches it) on n elements placed `offset` elements
 * into the device buffers (Adam refuses a base that is not 16-byte aligned).  p, m, v are updated in place from g with
 * the bias-corrected step size of step t (the network's adam_step_size), passed as an argument or, when lr_on_device, through
 * device memory as a captured train step passes it.  *lr_t = that step size. */
/* Test hook: one launch of the regularised optimiser step (p3d_opt_step, as adam_range launches it when a term is on) on n
 * elements placed `offset` (0..3) elements into the device buffers.  Tiles k = 0..ntile-1 cover [0, n) in order:
 * [tile_off[k], tile_off[k] + tile_len[k]) with coefficient tile_c[k].  g becomes g + c*p; with update, p, m, v take the Adam
 * step of step t on it (step size as p3d_debug_adam: argument or device memory), without it they stay as they are.
 * *term = sum_k 0.5 * c_k * sum(p^2) over tile k, in double, before the update.  *lr_t = the step size. */
int p3d_debug_adam_decay(int device, float* p, float* g, float* m, float* v, int64_t n, int offset, const int64_t* tile_off,
                         const int64_t* tile_len, const float* tile_c, int ntile, float lr, int64_t t, float b1, float b2, float eps,
                         int lr_on_device, int update, double* term, float* lr_t);
int p3d_debug_adam(int device, float* p, const float* g, float* m, float* v, int64_t n, int offset, float lr, int64_t t, float b1,
                   float b2, float eps, int lr_on_device, float* lr_t);
/* Test hooks: one Momentum or SGD launch (kind P3D_OPT_MOMENTUM / P3D_OPT_SGD, as the network's optimiser step launches it) on
 * n elements placed `offset` (0..3) elements into the device buffers; m is the accumulator (untouched by SGD).  The step size
 * lr is passed as an argument or, when lr_on_device, through device memory as a captured train step passes it.  The decay
 * variant is p3d_debug_adam_decay's launch with this update: g becomes g + c*p per tile, and with update p (and m) take the
 * step on it; *term as there. */
int p3d_debug_optimizer(int device, int kind, float* p, float* g, float* m, int64_t n, int offset, float lr, float momentum,
                        int use_nesterov, int lr_on_device);
int p3d_debug_optimizer_decay(int device, int kind, float* p, float* g, float* m, int64_t n, int offset, const int64_t* tile_off,
                              const int64_t* tile_len, const float* tile_c, int ntile, float lr, float momentum, int use_nesterov,
                              int lr_on_device, int update, double* term);
/* Test hook: one ema_kernel launch (p3d_set_ema; as the train step launches it) on n shadows s and parameters p placed `offset`
 * (0..3) elements past a 16-byte boundary of the device buffers; om is passed as an argument or, when om_on_device, through
 * device memory as a captured step with warm-up passes it.  The hook surrounds both ranges with guard elements and returns -1
 * if the launch changed one, or changed p. */
int p3d_debug_ema(int device, float* s, const float* p, int64_t n, int offset, float om, int om_on_device);
/* Test hook: one grad_accum_kernel launch (p3d_set_grad_accum; as the train step launches it) on n accumulator elements acc and
 * gradients g placed `offset` (0..3) elements past a 16-byte boundary of the device buffers.  mode 0 (STORE): acc = g; 1 (ADD):
 * acc = fadd(acc, g); 2 (FINISH): g = fadd(acc, g).  The operand the mode writes comes back in place.  The hook surrounds both
 * ranges with guard elements and returns -1 if the launch changed one, or changed the operand its mode must not write (g under
 * STORE and ADD, acc under FINISH). */
int p3d_debug_grad_accum(int device, int mode, float* acc, float* g, int64_t n, int offset);
/* Test hook: the augmentation launches of p3d_set_augment, as the step sends them, with EXPLICIT per-clip decisions: geom [B][6] =
 * flip, reverse, y0, x0, ch, cw and photo [B][2] = a, b, on x [B,T,H,W,3], y [B,T,H,W] and fix [B,T,H,W] bytes (NULL: no fixation
 * launch, fix_out is not written) of any T, H, W >= 1.  Every device buffer sits `offset` (0..3) elements -- bytes for the
 * fixations -- past a 16-byte boundary; offsets 1-3 force the element-by-element paths.  Guard elements surround every output:
 * the hook returns -1 if the launches changed one, or an input.  A window that leaves the frame is refused before any launch.
 * p3d_debug_augment_draw (host only, no HIP call): the decisions p3d_set_augment's settings *cfg give clip g under `seed` on
 * an H x W grid; -1 for settings p3d_set_augment refuses. */
int p3d_debug_augment(int device, const float* x, const float* y, const unsigned char* fix, int B, int T, int H, int W, const int32_t* geom,
                      const float* photo, int offset, float* x_out, float* y_out, unsigned char* fix_out);
int p3d_debug_augment_draw(uint64_t seed, uint64_t g, int H, int W, const p3d_augment* cfg, int32_t geom[6], float photo[2]);
/* Test hook: any of the optimiser launches above with clipping's scale (OptArgs::gscale, read from device memory): kind
 * P3D_OPT_*, ntile = 0 for the plain kernels (tile pointers and term may be NULL) or a tile table as p3d_debug_adam_decay takes
 * it; g becomes g + c*p (not scaled), the update runs on fmul(g', gscale).  t and the betas matter under Adam only, momentum
 * and use_nesterov under Momentum; v is not touched unless Adam.  *lr_t = the step size used. */
int p3d_debug_opt_scaled(int device, int kind, float* p, float* g, float* m, float* v, int64_t n, int offset, const int64_t* tile_off,
                         const int64_t* tile_len, const float* tile_c, int ntile, float lr, int64_t t, float b1, float b2, float eps,
                         float momentum, int use_nesterov, int lr_on_device, float gscale, double* term, float* lr_t);
/* Test hook: the global-norm reduction of p3d_set_grad_clip (grad_sumsq_kernel, launched from the description the step uses) on
 * n gradients g and, where a chunk has a coefficient, parameters p (NULL: none), placed `offset` (0..3) elements into the device
 * buffers.  Chunks k = 0..nchunk-1: [chunk_off[k], chunk_off[k] + chunk_len[k]) with coefficient chunk_c[k], ascending, without
 * overlap; elements in no chunk (slot padding) are not read.  The ranges [range_lo[r], range_hi[r]) are launched in the order
 * given, each over the chunks that start inside it, the last one folding; they must take every chunk exactly once.
 * max_blocks caps the grid (0: the step's cap).  Results as p3d_get_grad_norm's. */
int p3d_debug_grad_norm(int device, const float* g, const float* p, int64_t n, int offset, const int64_t* chunk_off,
                        const int64_t* chunk_len, const float* chunk_c, int nchunk, const int64_t* range_lo, const int64_t* range_hi,
                        int nrange, float clip_norm, int max_blocks, double* sumsq, double* norm, float* scale);
int p3d_debug_stat_parts(const int64_t xshape[5], const int64_t wshape[5], const int s[3], int transpose, int* written, int* cap);
int p3d_debug_igemm_groupable(const int64_t xshape[5], const int64_t wshape[5], const int s[3]);
int p3d_op_max_pool3d(int device, const float* x, const int64_t xshape[5], const int ksize[3], const int s[3], float* y);
int p3d_op_max_pool3d_grad(int device, const float* x, const int64_t xshape[5], const int ksize[3], const int s[3],
                           const float* dy, float* dx);
/* BiasAddGrad of tf.nn.bias_add (the bias of tf.layers.conv3d / conv3d_transpose, p3d.py:147-150): dbias[c] = sum over
 * rows of dy[row][c]; fixed summation order, bit-identical run to run. */
int p3d_op_bias_add_grad(int device, const float* dy, int64_t rows, int channels, float* dbias);
/* Test hooks: the conv launches in the forms the train step uses -- operands that are channel slices of wider rows, results added to
 * what the output holds, several filter gradients in one launch, the fp16 option -- built from the builders of the graph's conv ops.
 * Every OUTPUT buffer is in / out at its full extent: the caller decides what the kernels find there, and gets back every float.
 * A slice is `channels` floats at column `off` of rows of `ld` floats (all multiples of 4, off + channels <= ld).
 *
 * p3d_debug_conv_launch: kind 0 = tf.nn.conv3d forward (in = x, out = y), 1 = its input gradient (in = dy, out = dx; xshape is
 * the shape of x), 2 = tf.layers.conv3d_transpose forward (shapes as p3d_op_conv3d_transpose).  in [rows][ld_in], out
 * [rows][ld_out].  accum = 1: out += result (kinds 0, 1); the residue classes of a strided conv's input gradient that no tap reaches
 * are then not launched, and written (zeros; kind 2: the bias) otherwise.  f16 = 1: the fp16 option of p3d_set_pointwise_fp16,
 * 1x1x1 convs of kinds 0 and 1 only.  bias: kinds 0 and 2, or null.  kernels: the names the launches went out under, joined
 * with ';' ("(tail)" appended where a single launch sends its last round K-sliced); splits (or null): the smallest and the largest
 * K-slice count of the launches' plans, which the names do not carry.  The stem shape is refused.
 *
 * p3d_debug_wgrad_group: n (1..6) filter gradients as ONE launch, as the step's queue sends them.  Per problem i: x[i] [rows][ldx[i]],
 * xshape xs[5 i ..], dy[i] [rows][lddy[i]], filter shape ws[5 i ..], strides s[3 i ..]; transpose[i] = 1: the problem is a
 * transposed conv's (shapes as p3d_op_conv3d_transpose, x its input, dy the gradient of its output).  dw[i] (in / out) and dbias[i]
 * (in / out, or null) are ADDED to.  polite / greedy: the residency flags of the launch.  kernel: its name; cuts[i]: the cuts of
 * problem i along the positions (0: the problem has no positions or taps and is dropped); info = slab stride (the largest cut
 * count), tile rows, tile columns.
 *
 * p3d_debug_max_pool3d(_grad), p3d_debug_bias_add_grad: p3d_op_max_pool3d(_grad) / p3d_op_bias_add_grad on slices; y, dx and
 * dbias in / out; accumulate = 1: dx += the gradient; *kernel = the backward kernel that ran. */
int p3d_debug_conv_launch(int device, int kind, const float* in, int ld_in, int off_in, const int64_t xshape[5], const float* w,
                          const int64_t wshape[5], const int s[3], const float* bias, int accum, int f16, float* out, int ld_out,
                          int off_out, char* kernels, int kernels_cap, int* splits);
int p3d_debug_wgrad_group(int device, int n, const float* const* x, const int* ldx, const int* offx, const int64_t* xs,
                          const float* const* dy, const int* lddy, const int* offdy, const int64_t* ws, const int* s, const int* transpose,
                          float* const* dw, float* const* dbias, int polite, int greedy, char* kernel, int kernel_cap, int* cuts,
                          int* info);
/* Test hooks: the fused-BatchNorm launches of the bottleneck convs (p3d_set_bn_fusion) -- operand transforms, coefficient folds,
 * gated epilogues, finalize launches -- built by the builders conv() uses, on host arrays.  Slices as above.  Every array a launch
 * may WRITE is in / out at its full extent: the caller prefills it and gets every float back, touched or not.
 *
 * p3d_fused_bn: one BatchNorm source of a RELU1 / RELU2 operand.  y [rows of the conv's input][ld], the raw tensor the BatchNorm
 * normalises, `channels of the conv's input` floats at column off (two sources that name the SAME y pointer share one device
 * buffer).  partials [nparts][C][2] (sum, sum of squares) over `rows` rows, or null: the launch reads scale / shift as given.
 * With partials: publish = 1 makes block 0 of slice 0 (or, above P3D_FOLD_MAX = 32 partials, a bn_finalize_kernel launch) write
 * scale, shift, mean, invstd [C] and, with update_moving, the moving statistics; publish = 0 writes none of them.
 *
 * p3d_fused_bn_grad: the BatchNorm a GRAD operand differentiates through.  y [rows of the conv's output][ld]: the BatchNorm's input
 * (the conv's own output); gamma, mean, invstd [Cout].  partials [nparts][Cout][2] (sum g, sum g*xhat) over `rows` rows with
 * publish (coef [3][Cout], dgamma, dbeta [Cout] written; above 32 partials by a bn_grad_finalize_kernel launch), or null: coef read.
 *
 * p3d_fused_gate: one gate of the epilogue.  y [rows of the conv's input][ld_y] and scale, shift, mean, invstd [Cin] are read;
 * out [rows][ld_out] receives the gated gradient; part [part_rows][Cin][2] the per-tile-row (sum g, sum g*xhat): the launch must
 * need at most part_rows rows (checked before it goes out).
 *
 * p3d_fused_conv: kind 0 = forward with at = 1 (RELU1) or 2 (RELU2) on src[]; out = the conv's output.  kind 1 = input gradient:
 * g [rows of the conv's output][ld_g] the gradient of that output, out = the raw result buffer (written when there is no gate or
 * raw_store = 1, read when accum = 1), grad = 1: the GRAD transform of g by gbn; ngate gates.  xshape = shape of the conv's input.
 * Returned in the struct: gpart_rows = rows of gradient partials every gate received.  kernels / splits as p3d_debug_conv_launch.
 *
 * p3d_debug_fused_wgrad: as p3d_debug_wgrad_group; per problem i additionally xt[i] = 0 / 1 / 2 with xs1 / xt1 [Cin] (and x2 with
 * ldx2 / offx2, xs2, xt2 for xt = 2), dyt[i] = 0 / 1 with dy2 [rows][lddy2] at offdy2 and dcoef [3][Cout].
 *
 * p3d_debug_fused_reject: the launcher's answer (a hipError_t; *validator: the filter gradient validator's, 1 = takes it) to malformed
 * fused launches, which must never go out.  which: 0 / 1 RELU1 with 0 / 33 partials, 2 / 3 GRAD with 0 / 33, 4 a gate beside a
 * statistics sink, 5 RELU1 with transposed weights, 6 RELU2 with a second row length that is no multiple of 4, 7 xt with pair,
 * 8 xt = 2 with such a row length, 9 dyt with pair. */
typedef struct p3d_fused_bn {
    const float* y; int ld, off;
    const float* gamma; const float* beta;
    const float* partials; int nparts; int64_t rows; int publish, update_moving;
    float* scale; float* shift; float* mean; float* invstd;
    float* moving_mean; float* moving_var;
} p3d_fused_bn;
typedef struct p3d_fused_bn_grad {
    const float* y; int ld, off;
    const float* gamma; const float* mean; const float* invstd;
    const float* partials; int nparts; int64_t rows; int publish;
    float* coef; float* dgamma; float* dbeta;
} p3d_fused_bn_grad;
typedef struct p3d_fused_gate {
    const float* y; int ld_y, off_y;
    const float* scale; const float* shift; const float* mean; const float* invstd;
    float* out; int ld_out, off_out;
    float* part; int part_rows;
} p3d_fused_gate;
typedef struct p3d_fused_conv {
    int kind;
    int64_t xshape[5]; int64_t wshape[5]; int stride[3];
    const float* w; const float* bias; int f16;
    int at; p3d_fused_bn src[2];
    const float* g; int ld_g, off_g;
    int grad; p3d_fused_bn_grad gbn;
    int ngate; p3d_fused_gate gate[2]; int raw_store, accum;
    float* out; int ld_out, off_out;
    int gpart_rows;
} p3d_fused_conv;
int p3d_debug_fused_conv(int device, p3d_fused_conv* a, char* kernels, int kernels_cap, int* splits);
int p3d_debug_fused_wgrad(int device, int n, const float* const* x, const int* ldx, const int* offx, const int64_t* xs,
                          const float* const* dy, const int* lddy, const int* offdy, const int64_t* ws, const int* s,
                          const int* xt, const float* const* x2, const int* ldx2, const int* offx2, const float* const* xs1,
                          const float* const* xt1, const float* const* xs2, const float* const* xt2, const int* dyt,
                          const float* const* dy2, const int* lddy2, const int* offdy2, const float* const* dcoef,
                          float* const* dw, float* const* dbias, char* kernel, int kernel_cap, int* cuts, int* info);
int p3d_debug_fused_reject(int device, int which, int* error, int* validator);
int p3d_debug_max_pool3d(int device, const float* x, int ldx, int offx, const int64_t xshape[5], const int ksize[3], const int s[3],
                         float* y, int ldy, int offy);
int p3d_debug_max_pool3d_grad(int device, const float* x, int ldx, int offx, const int64_t xshape[5], const int ksize[3], const int s[3],
                              const float* dy, int ldy, int offy, int accumulate, float* dx, const char** kernel);
int p3d_debug_bias_add_grad(int device, const float* dy, int64_t rows, int channels, int ld, int off, float* dbias);
/* The core of attention(), utils/network.py:183-185, on flattened operands:
 *     s = tf.matmul(hw_flatten(g), hw_flatten(f), transpose_b=True); beta = tf.nn.softmax(s); o = tf.matmul(beta, hw_flatten(h))
 * g [batch][n_g][ch/8], f [batch][n_f][ch/8], h [batch][n_f][ch] -> o [batch][n_g][ch], on the kernels that keep the score
 * matrix on chip (ch in {32, 64, 128, 256}).  With d_o (the gradient of o) it also writes dg, df, dh. */
int p3d_op_attention_core(int device, int batch, int n_g, int n_f, int ch, const float* g, const float* f, const float* h,
                          float* o, const float* d_o, float* dg, float* df, float* dh);
/* Test hooks: the self-attention block's kernels as the train step launches them (tests/test_gpu_attention.py).
 *
 * p3d_debug_attention_core: p3d_op_attention_core in either execution of p3d_set_attention_mode.  mode 1: the stored-score
 * sequence of the graph op (row padding of f and h to a multiple of 4 keys, per-clip GEMMs on the conv kernels, softmax rows,
 * filter-gradient launches for df and dh) on buffers of its own; any ch that is a multiple of 32.  mode 2: the kernels that keep
 * the scores on chip; ch in {32, 64, 128, 256}, anything else is refused.  Every output buffer, the stored scores and every scratch
 * buffer holds NaNs before the launches.
 * p3d_debug_attention_splits (host only): K-slices the plan gives the four row-major products of mode 1 at this shape, in launch
 * order: g f^T, beta h, d_o h^T, ds f (1: not sliced).
 *
 * p3d_debug_softmax_rows: softmax over the first `cols` floats of rows of `ld` floats, in place (backward = 0: s becomes the
 * attention map, columns [cols, ld) zero), or its gradient (backward = 1: s = the attention map, d = its gradient on entry and the
 * gradient of the scores on return, columns [cols, ld) zero).  s and d are [rows + guard_rows][ld], copied in and back whole: the
 * guard rows after the last row must come back as they went in.
 *
 * p3d_debug_attn_mix: z = r * gamma + x over M rows of C channels (utils/network.py:191), with the block's dropout of rate
 * drop_rate (0: none) keyed by seed -- passed as an argument, or read from device memory when seed_dev -- and, with dz, the
 * backward pass.  r / dr are C channels at column offr of rows of ldr floats, x / dx at offx of ldx, z / dz at offz of ldz.  z, dr
 * and dx are in / out at their full extent [M][ld]; accx = 1: dx += the gradient; dgamma[1] is added to. */
int p3d_debug_attention_core(int device, int mode, int batch, int n_g, int n_f, int ch, const float* g, const float* f, const float* h,
                             float* o, const float* d_o, float* dg, float* df, float* dh);
int p3d_debug_attention_splits(int batch, int n_g, int n_f, int ch, int splits[4]);
int p3d_debug_softmax_rows(int device, int backward, int64_t rows, int cols, int ld, float* s, float* d, int guard_rows);
int p3d_debug_attn_mix(int device, int64_t M, int C, const float* r, int ldr, int offr, const float* x, int ldx, int offx, float gamma,
                       float drop_rate, uint64_t seed, int seed_dev, float* z, int ldz, int offz, const float* dz, int accx, float* dr,
                       float* dx, float* dgamma);

/* ---- validation metrics and frame pre-processing: the steps either side of the path.
 *      Host arrays in and out, float64 results.  Maps are float32 [n_maps][n_pix] of ONE shape (the reference's
 *      resize-to-match branch is not on the trainers' path).  Reference: utils/metrics.py. */
int p3d_metric_cc(int device, const float* map1, const float* map2, int n_maps, int n_pix, double* out);    /* CC, utils/metrics.py:227-250 */
int p3d_metric_sim(int device, const float* map1, const float* map2, int n_maps, int n_pix, double* out);   /* SIM, :258-287 */
int p3d_metric_nss(int device, const float* sal, const float* fix, int n_maps, int n_pix, double* out);     /* NSS, :200-224; fix > 0.5 */
/* AUC_Judd, utils/metrics.py:25-85.  jitter: the noise the reference adds (random.rand * 1e-7, :62-63) supplied by the
 * caller, [n_maps][n_pix], or NULL for jitter=False.  NaN where a map has no fixation. */
int p3d_metric_auc_judd(int device, const float* sal, const float* fix, const float* jitter, int n_maps, int n_pix, double* out);
/* AUC_Borji, utils/metrics.py:88-154, one map.  rand_idx = the reference's r = random.randint(0, n_pix, [n_fix, n_rep])
 * (:139), row-major; n_fix must equal the number of pixels with fix > 0.5.  out[n_rep] = area per random split (the
 * reference returns their mean). */
int p3d_metric_auc_borji(int device, const float* sal, const float* fix, const int* rand_idx, int n_pix, int n_fix, int n_rep,
                         double step_size, double* out);
/* mapf, dataflow.py:198-216: n decoded BGR uint8 frames [n][H0][W0][3] -> RGB - mean_rgb -> cv2.INTER_LINEAR resize to
 * H x W -> / 255, float32 [n][H][W][3] (one clip of the NDHWC input); and the grey density maps [n][H0][W0] -> [n][H][W]. */
int p3d_mapf_frames(int device, const unsigned char* bgr, int n, int H0, int W0, const float mean_rgb[3], int H, int W, float* out);
int p3d_mapf_density(int device, const unsigned char* grey, int n, int H0, int W0, int H, int W, float* out);

/* ---- the evaluation pass of test.py (test.py:160-183): metrics at ground-truth resolution, whole-GPU reductions.
 * cv2.resize(map, (W, H), INTER_LINEAR) of float32 maps [n][h][w] -> [n][H][W] (test.py:170), bit-exact to the float32 path
 * of OpenCV's generic resize (no FMA). */
int p3d_resize_linear(int device, const float* src, int n, int h, int w, int H, int W, float* dst);
/* AUC_shuffled, utils/metrics.py:157-197, one map: AUC_Borji's per-split sweep with S_rand = S at other_idx [n_rand][n_rep]
 * (the pixels of the other maps' fixations the caller drew, row-major), n_rand = min(n_fix, fixated pixels of other_map);
 * the false-positive rate still divides by n_fix (:151-152).  n_fix must equal the count of fix > 0.5.  out[n_rep] = area
 * per split, NaN when nothing is fixated. */
int p3d_metric_auc_shuffled(int device, const float* sal, const float* fix, const int* other_idx, int n_pix, int n_fix, int n_rand,
                            int n_rep, double step_size, double* out);
/* CC, SIM, AUC_Judd, AUC_Borji, NSS (out[B][5], in test.py:172-176's order) of the LAST frame of every clip of the handle's last
 * forward pass, all on the device:
 *   prediction [B][T][h][w] frame T-1 -> cv2.INTER_LINEAR float32 resize to H x W (test.py:170);
 *   density [B][Hd][Wd] uint8 -> the uint8 resize to H x W (p3d_mapf_density's path), / 255. in double (dataflow.py:236-238);
 *   fixation [B][H][W] uint8, fixated <=> / 255. > 0.5 <=> byte >= 128 (dataflow.py:239-241).
 * jitter [B][H][W] (or NULL: jitter=False) is AUC_Judd's noise random.rand(H, W) * 1e-7 in float64; it is added to the
 * prediction in double and rounded once to float32, in place as utils/metrics.py:65 does, so AUC_Borji and NSS see the
 * jittered map and CC / SIM the clean one.  (p3d_metric_auc_judd takes float32 noise and adds it in float32.)
 * borji_idx = the clips' randint(0, H*W, [n_fix_b, n_rep]) draws, concatenated; n_fix[B] = the host's fixation counts: a count
 * that disagrees with the device's is refused.  Clips without fixation give NaN for AUC_Judd, AUC_Borji and NSS.
 * stage_ms[2] (or NULL): device time of the host->device copies and of the metric stage (resizes included). */
int p3d_eval_last_frames(p3d_handle* h, const unsigned char* density, int Hd, int Wd, const unsigned char* fixation, int H, int W,
                         const double* jitter, const int* borji_idx, const int* n_fix, int n_rep, double step_size, double* out,
                         double* stage_ms);
/* Test hook: the launches of p3d_eval_last_frames (one shared sequence: uploads, float32 resize, density, the metric passes,
 * read-back, the n_fix check) on maps the caller supplies instead of the handle's prediction.  maps [n_maps][h][w][elem_stride]
 * float32, channel 0 is scored (elem_stride > 1: how the prediction buffer is addressed); density [n_maps][Hd][Wd], fixation
 * [n_maps][H][W], jitter, borji_idx, n_fix[n_maps] and out[n_maps][5] as above (tests/test_gpu_eval_maps.py). */
int p3d_debug_eval_maps(int device, const float* maps, int n_maps, int h, int w, int elem_stride, const unsigned char* density,
                        int Hd, int Wd, const unsigned char* fixation, int H, int W, const double* jitter, const int* borji_idx,
                        const int* n_fix, int n_rep, double step_size, double* out);

/* ---- gen_pred.py's write-out (gen_pred.py:154-168): every emitted 112x112 map as an 8-bit image at 1080x960.
 * cv2.imwrite(name, cv2.resize(float64(map * 255.), (W, H))) per map: the float32 product map * scale widened to double,
 * INTER_LINEAR on CV_64F (the float32 path's coordinates and float32 weights, double arithmetic, no FMA; same size: a copy),
 * then imwrite's saturate_cast<uchar>: round half to even, clamp to [0, 255]; NaN and rounded values outside int32 give 0
 * (x86 OpenCV; the reference's semantics are pinned for |v| < 2^31 only).  H * W <= INT32_MAX.
 * Host arrays [n][h][w] float32 -> [n][H][W] uint8 (op level, tests). */
int p3d_resize_linear_u8(int device, const float* src, int n, int h, int w, float scale, int H, int W, unsigned char* dst);
/* The same on the handle's last prediction (p3d_predict_windows / p3d_forward), [B][T][h][w]: clip b's frames first_frame[b] ..
 * T-1, packed in clip order then frame order into out[sum(T - first_frame[b])][H][W].  first_frame[b] = 0 is the first
 * window (all 16 maps, gen_pred.py:154-160), 15 a later one (its newest frame, :161-168), T a clip that writes nothing (the
 * padding of a short last batch).  Refuses first_frame outside [0, T] and a handle that has run no forward pass.  Scratch
 * from the stream pool.  stage_ms[2] (or NULL): device time of the resize / quantise stage and of the device->host copy. */
int p3d_pred_maps_u8(p3d_handle* h, const int* first_frame, float scale, int H, int W, unsigned char* out, double* stage_ms);

/* ---- Gaussian smoothing and per-map normalisation of predictions at output resolution (an ADDITION: gen_pred.py writes map * 255
 * and test.py scores the bare resize; the reference's ground-truth densities are smoothed this way, gen_video.py:15, and
 * utils/metric_utils.py normalises by 'range').  OFF by default; off, every entry point issues what it issued before and returns
 * the same bits.  PARITY UNPINNED: cv2 is not available to the tests, so this text is the contract and tests/postprocess_ref.py
 * replays it in numpy bit for bit.  One map of H x W float32 values v goes through:
 *   RADIUS  radius > 0 is taken as given.  radius == 0 and sigma > 0: cv2's rule for float images,
 *           ksize = (int)rint(8.0 * sigma + 1.0) | 1, r = ksize / 2, in double on the float32 sigma (sigma 32 -> r 128, 1 -> 4).
 *           sigma == 0: no blur (r = 0).  r <= P3D_BLUR_MAX_RADIUS.
 *   TAPS    e_k = exp(-(k - r)^2 / (2 sigma^2)) in double, k = 0 .. 2r;  S = sum of e_k in ascending k, in double;
 *           w_k = (float)(e_k / S).  p3d_blur_taps returns these 2r + 1 floats and r (host only; cap = room in taps, in floats).
 *   PASS    along an axis of length n, in float32, no fused multiply-add, every operation rounded on its own:
 *           acc = fmul(w_r, s[i]);  for d = 1 .. r:  acc = fadd(acc, fmul(w_{r+d}, fadd(s[rho(i - d)], s[rho(i + d)])));
 *           rho is reflect-101: rho(j) = -j for j < 0, 2 (n - 1) - j for j > n - 1.  Needs r <= n - 1.
 *   BLUR    the pass along x over the whole map into a temporary, then the pass along y over the temporary.  fadd commutes, so
 *           the blur commutes bit for bit with a horizontal or a vertical flip.
 *   NORM    after the blur, with mn and mx the float32 minimum and maximum of the map:
 *           P3D_NORM_MAX    v' = v / mx when mx > 0, else the map is left as it is;
 *           P3D_NORM_RANGE  v' = (v - mn) / (mx - mn) when mx > mn, else every element becomes 0;
 *           float32 subtraction and division, correctly rounded.
 *   BYTE    where bytes are asked for: saturate_cast<uchar>((double)fmul(v', scale)), p3d_resize_linear_u8's byte law.
 * Maps that hold NaN or inf propagate them; their results (and the sign of a zero minimum) are NOT pinned.
 * Refused (-1, p3d_last_error set, nothing changed): sigma negative or not finite; radius < 0 or > P3D_BLUR_MAX_RADIUS (also the
 * radius that follows from sigma); radius > 0 with sigma == 0; an unknown norm; and, when the stage runs, r > min(H, W) - 1.
 *
 * p3d_set_postprocess: the handle's setting; NULL or {0, 0, P3D_NORM_NONE} switch it off.  Nothing is allocated until the stage
 * first runs (scratch from the stream pool); the train step, a captured step graph and its schedule never see it.  While on:
 *   p3d_eval_last_frames  the stage runs on the float32 resize of the prediction, in place, before the jitter is added and before
 *                         every metric: all five metrics score the smoothed, normalised map;
 *   p3d_pred_maps_u8      every emitted map is resized to H x W by p3d_resize_linear's FLOAT32 law (not the double-precision
 *                         resize of the option-off path: the chain is the one evaluation uses, and smoothing belongs at output
 *                         resolution), then BLUR, NORM, BYTE.  Maps are processed 16 at a time: scratch is 2 x 16 x H x W floats
 *                         (at 1080x960 a first window's 16 maps of 4 MB each, plus the temporary: 133 MB) beside the bytes.
 * p3d_get_postprocess: the setting (zeros while off) and whether it is on; either pointer may be NULL.
 * p3d_gaussian_blur: BLUR alone on host maps src [n][H][W] -> dst [n][H][W].
 * p3d_postprocess_maps: the same launch sequence (resize, BLUR, NORM, BYTE) on host maps [n][h][w][elem_stride], channel 0;
 * out_f32 [n][H][W] and out_u8 [n][H][W] may each be NULL (scale is read for out_u8 only); cfg NULL or neutral: the float32 resize
 * alone.  Its outputs sit between guard elements on the device, out_u8 at an odd offset; a guard that changed is an error.
 * p3d_debug_eval_maps_post: p3d_debug_eval_maps with the stage of cfg (NULL: off) between the resize and the metrics. */
enum { P3D_NORM_NONE = 0, P3D_NORM_MAX = 1, P3D_NORM_RANGE = 2 };
#define P3D_BLUR_MAX_RADIUS 255
typedef struct p3d_postprocess { float sigma; int radius; int norm; } p3d_postprocess;
int p3d_set_postprocess(p3d_handle* h, const p3d_postprocess* cfg);
int p3d_get_postprocess(p3d_handle* h, p3d_postprocess* cfg, int* on);
int p3d_blur_taps(float sigma, int radius, float* taps, int cap, int* r);
int p3d_gaussian_blur(int device, const float* src, int n, int H, int W, float sigma, int radius, float* dst);
int p3d_postprocess_maps(int device, const float* maps, int n, int h, int w, int elem_stride, int H, int W,
                         const p3d_postprocess* cfg, float scale, float* out_f32, unsigned char* out_u8);
int p3d_debug_eval_maps_post(int device, const float* maps, int n_maps, int h, int w, int elem_stride, const unsigned char* density,
                             int Hd, int Wd, const unsigned char* fixation, int H, int W, const double* jitter, const int* borji_idx,
                             const int* n_fix, int n_rep, double step_size, double* out, const p3d_postprocess* cfg);
/* Host only (no HIP call): the vertical pass's strip for radius r -- columns, output rows and LDS bytes of one block. */
int p3d_debug_blur_strip(int r, int* cols, int* rows, int* lds_bytes);

/* ---- Histogram matching of predictions at output resolution (utils/metric_utils.py:56-84 match_hist(image, cdf, bin_centers,
 * nbins=256), on tables made by skimage's exposure.cumulative_distribution; the reference's recipe, :321, is
 * match_hist(map1, *exposure.cumulative_distribution(map2))).  It remaps a map so that its histogram follows a target's.  OFF by
 * default; off, every entry point issues what it issued before and returns the same bits.  PARITY UNPINNED: skimage is not
 * available to the tests, so this text is the contract; it is np.histogram plus np.interp, tests/hist_match_ref.py replays it in
 * numpy bit for bit, and tests/test_hist_match_cpu.py holds that replay to numpy's own two functions.
 * Everything is float64 on the float32 inputs, no fused multiply-add, every operation rounded on its own.  nb is the bin count,
 * 2 <= nb <= P3D_HIST_MAX_BINS, 256 where a default applies.
 *   CDF     of one map a of N values (np.histogram(a, nb), cumsum, / N):  mn, mx the map's minimum and maximum; if mn == mx they
 *           become mn - 0.5 and mx + 0.5.  step = (mx - mn) / nb;  edge[k] = mn + k * step for k < nb, edge[nb] = mx;
 *           norm = nb / (mx - mn).  The bin of v, in this order:  i = (int)((v - mn) * norm);  if i == nb: i = nb - 1;
 *           if v < edge[i]: i -= 1;  else if v >= edge[i + 1] and i != nb - 1: i += 1.  count[k] is an integer;
 *           centre[k] = (edge[k] + edge[k + 1]) / 2;  cdf[k] = (double)(count[0] + ... + count[k]) / (double)N, the running sum
 *           kept in integers.
 *   INTERP  interp(x, xp, fp) over n entries, xp non-decreasing (np.interp):  x < xp[0]: fp[0];  x >= xp[n - 1]: fp[n - 1];  else
 *           with j the largest index with xp[j] <= x:  fp[j] if x == xp[j], otherwise
 *           ((fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j])) * (x - xp[j]) + fp[j].
 *   MATCH   of a source map against a target table (cdf_t, centre_t) of nt entries:  new[k] = interp(cdf_s[k], cdf_t, centre_t)
 *           for k < nb;  out = (float)interp((double)v, centre_s, new) per pixel, rounded to float32 once.
 * Maps that hold NaN or inf are NOT pinned (they stay inside every buffer).  Supplied tables are checked on the host.
 * Refused (-1, p3d_last_error set, nothing changed): nbins or nt outside [2, P3D_HIST_MAX_BINS]; a table that is not finite and
 * non-decreasing (cdf and centres both); an unknown mode; NULL tables under P3D_MATCH_TABLE.
 *
 * p3d_cumulative_distribution  CDF on host maps [n][H][W] -> cdf [n][nbins], centres [n][nbins], and the counts [n][nbins] as
 *                      int64 unless counts is NULL.
 * p3d_match_hist       the reference's function: MATCH of maps [n][H][W] against n_tables (1, or n: one per map) tables of nt
 *                      entries, cdf_t / centre_t [n_tables][nt] -> out [n][H][W].
 * p3d_match_hist_maps  the reference's recipe: every map matched to the table of its own target image targets [n][H][W], both
 *                      tables built on the device (nt = nbins).
 * p3d_set_hist_match   the handle's setting, separate from p3d_set_postprocess; NULL or mode P3D_MATCH_OFF switch it off.  The
 *                      tables are copied at set time.  Nothing is allocated until the stage first runs (scratch from the stream
 *                      pool); the train step, a captured step graph and its schedule never see it.  The stage sits between BLUR
 *                      and NORM of p3d_set_postprocess's chain: resize -> BLUR -> MATCH -> NORM -> BYTE (p3d_set_prior_stage's
 *                      stage, further down, goes between BLUR and MATCH).
 *     P3D_MATCH_TABLE    one supplied table for every map, in p3d_eval_last_frames, p3d_pred_maps_u8 and p3d_video_maps_u8.
 *                        With p3d_set_postprocess off, the two byte writers take the float32-resize chain, as they do for the blur.
 *     P3D_MATCH_DENSITY  evaluation only: each prediction is matched to the table of its own ground-truth density at H x W, the
 *                        doubles b / 255. of the resized bytes b that the metrics use, before the jitter is added and before
 *                        every metric.  p3d_pred_maps_u8 and p3d_video_maps_u8 refuse while this mode is set.
 * p3d_get_hist_match   mode, nbins (0 while off), nt and pointers to the handle's copy of the table (NULL without one; valid
 *                      until the next p3d_set_hist_match or p3d_destroy).
 * p3d_postprocess_maps_match  p3d_postprocess_maps with the stage of `match` (NULL: off; P3D_MATCH_DENSITY is refused).
 * p3d_debug_eval_maps_match   p3d_debug_eval_maps_post with the stage of `match` (NULL: off). */
enum { P3D_MATCH_OFF = 0, P3D_MATCH_TABLE = 1, P3D_MATCH_DENSITY = 2 };
#define P3D_HIST_MAX_BINS 1024
typedef struct p3d_hist_match { int mode; int nbins; int nt; const double* cdf; const double* centres; } p3d_hist_match;
int p3d_cumulative_distribution(int device, const float* maps, int n, int H, int W, int nbins, int64_t* counts /* may be NULL */,
                                double* cdf, double* centres);
int p3d_match_hist(int device, const float* maps, int n, int H, int W, int nbins, const double* cdf_t, const double* centre_t,
                   int n_tables, int nt, float* out);
int p3d_match_hist_maps(int device, const float* maps, const float* targets, int n, int H, int W, int nbins, float* out);
int p3d_set_hist_match(p3d_handle* h, const p3d_hist_match* cfg);
int p3d_get_hist_match(p3d_handle* h, p3d_hist_match* cfg);
int p3d_postprocess_maps_match(int device, const float* maps, int n, int h, int w, int elem_stride, int H, int W,
                               const p3d_postprocess* cfg, const p3d_hist_match* match, float scale, float* out_f32,
                               unsigned char* out_u8);
int p3d_debug_eval_maps_match(int device, const float* maps, int n_maps, int h, int w, int elem_stride, const unsigned char* density,
                              int Hd, int Wd, const unsigned char* fixation, int H, int W, const double* jitter, const int* borji_idx,
                              const int* n_fix, int n_rep, double step_size, double* out, const p3d_postprocess* cfg,
                              const p3d_hist_match* match);

/* ---- KL divergence and information gain at scoring resolution (utils/metrics.py:338-362 KLdiv, the one function of that file
 * the evaluation pass did not have; and the MIT saliency benchmark's InfoGain(saliencyMap, fixationMap, baselineMap), an ADDITION
 * without a reference counterpart).  OFF by default; off, every entry point issues what it issued before and returns the same
 * bits; on, the five columns of p3d_eval_last_frames are still bit for bit what they are off.  PARITY UNPINNED: neither scipy nor
 * the MIT code is available to the tests, and the reference computes KLdiv in float32 with numpy's pairwise sum, which is not
 * reproduced: this text is the contract and tests/kl_ig_ref.py replays it in numpy float64; the kernels are held to that replay.
 * Per map of n = H * W elements, all arithmetic in float64, no fused multiply-add:
 *   s_i  the evaluation pass's CLEAN prediction widened to double: the float32 map after the resize and the optional BLUR / MATCH /
 *        NORM stages, before AUC_Judd's jitter -- the map CC and SIM see.
 *   y_i  the density: in the evaluation pass rint(q * 255) / 255 of the float32 density q, i.e. byte / 255. in double, what CC and
 *        SIM use; in the op-level entry points the supplied float32 widened to double.
 *   f_i  fixated <=> byte >= 128 (evaluation), fix > 0.5f (op level).
 *   eps  = 2.2204e-16, the reference's literal (not DBL_EPSILON).
 *   KLDIV      (utils/metrics.py:338-362; its scipy.misc.imresize to the other map's shape is taken as the identity on maps of
 *              one shape, and imresize's byte quantisation is deliberately not reproduced.)
 *              S1 = sum of s_i,  S2 = sum of y_i;   p_i = s_i / S1 if any s_i != 0, else s_i;   q_i = y_i / S2 if any y_i != 0,
 *              else y_i;   KL = sum of q_i * log(eps + q_i / (p_i + eps)).
 *              Nothing else is special-cased: an all-zero density gives 0, a NaN anywhere gives NaN, a negative p_i + eps gives
 *              NaN through log as in numpy.
 *   INFO GAIN  the baseline b is ONE float32 map [H][W] shared by all maps of a call (a centre prior, the mean training density).
 *              u_i = (s_i - min s) / (max s - min s);   P_i = u_i / U with U = (S1 - n * min s) / (max s - min s), the way the
 *              per-map loss forms its range sums;   B_i from b in the same way;
 *              IG = (1 / F) * sum over fixated i of (log2(eps + P_i) - log2(eps + B_i)),  F = the number of fixated elements.
 *              NaN when F = 0, when s or b is constant, or when either holds a NaN (the cases in which NSS and SIM are NaN).
 *   ORDER      every sum (S1, S2, the sums of b, KL's and IG's terms, F) is formed in full_pass_a's order: the map is cut into
 *              p3d_full_blocks(n) equal chunks, one per block; lane t of a block's 256 adds elements t, t + 256, ... of its chunk in
 *              ascending order; the 256 lane sums go through the block's halving tree (lane t += lane t + 128, then + 64, ...); the
 *              last arriving block adds the blocks' sums, lane t taking blocks t, t + 256, ..., then the same tree.  Minima and
 *              maxima likewise.  No floating-point atomics: the same bits on every run.
 * p3d_set_eval_extra   the handle's setting: flags = P3D_EVAL_KLDIV | P3D_EVAL_INFO_GAIN.  The baseline [H][W] is required if and
 *                      only if P3D_EVAL_INFO_GAIN is set; it is checked on the host (finite, not constant), copied to the device,
 *                      and its minimum, maximum and sum are taken there by one launch, once.  flags = 0 switches off and frees.
 *                      Refused (-1, p3d_last_error set, nothing changed): unknown flags, a missing or a superfluous baseline, a
 *                      baseline that is not finite or constant.  The train step, a captured step graph and its schedule never see it.
 *                      While on, p3d_eval_last_frames issues ONE more launch after pass A, on the scored map.
 * p3d_get_eval_extra   the flags, a pointer to the handle's copy of the baseline (NULL without one; valid until the next
 *                      p3d_set_eval_extra or p3d_destroy) and its size; every pointer may be NULL.
 * p3d_last_eval_extra  out[B][2] = KL, IG of the last p3d_eval_last_frames; a metric that is off reports NaN.  cap = room in out, in
 *                      doubles.  Refused: the option is off; no evaluation has run since it was set; the last evaluation's H x W
 *                      is not the baseline's (that evaluation ran without the launch; its five columns are unaffected).
 * p3d_debug_eval_maps_extra  p3d_debug_eval_maps_match with the launch of `flags` and a baseline [H][W] (NULL without
 *                      P3D_EVAL_INFO_GAIN); extra[n_maps][2] = KL, IG (may be NULL when flags = 0).
 * p3d_metric_kldiv     KLDIV of host maps [n_maps][n_pix], map1 the saliency map and map2 the density; beside p3d_metric_cc.
 * p3d_metric_info_gain INFO GAIN of host maps sal, fix [n_maps][n_pix] against baseline [n_pix]. */
enum { P3D_EVAL_KLDIV = 1, P3D_EVAL_INFO_GAIN = 2 };
int p3d_set_eval_extra(p3d_handle* h, int flags, const float* baseline, int H, int W);
int p3d_get_eval_extra(p3d_handle* h, int* flags, const float** baseline, int* H, int* W);
int p3d_last_eval_extra(p3d_handle* h, double* out /* [B][2]: KL, IG */, int64_t cap);
int p3d_debug_eval_maps_extra(int device, const float* maps, int n_maps, int h, int w, int elem_stride, const unsigned char* density,
                              int Hd, int Wd, const unsigned char* fixation, int H, int W, const double* jitter, const int* borji_idx,
                              const int* n_fix, int n_rep, double step_size, double* out, const p3d_postprocess* cfg,
                              const p3d_hist_match* match, int flags, const float* baseline, double* extra);
int p3d_metric_kldiv(int device, const float* map1, const float* map2, int n_maps, int n_pix, double* out);
int p3d_metric_info_gain(int device, const float* sal, const float* fix, const float* baseline, int n_maps, int n_pix, double* out);

/* ---- Fixation priors built on the device (an ADDITION without a reference counterpart: the MIT benchmark's information-gain
 * baseline is the fixation maps of the other images of a set, summed and smoothed, and gen_video.py:15 only names the sigma32
 * densities that were made this way).  The same map is the usual centre-bias correction of a saliency model.  OFF by default; off,
 * every entry point issues what it issued before and returns the same bits, and nothing is allocated.  The train step, a captured
 * step graph and its schedule never see any of it.  PARITY UNPINNED: this text is the contract and tests/prior_ref.py replays it in
 * numpy; the kernels are held to that replay bit for bit.
 *   COUNT   one accumulator per handle: count[H][W] of uint32 and the number of maps in it.  A map of H x W bytes adds, per pixel,
 *           1 where the byte is >= 128 (P3D_PRIOR_FIXATIONS, the evaluation pass's "fixated" rule) or the byte itself
 *           (P3D_PRIOR_BYTES, for 8-bit densities), times sign: +1 adds maps, -1 takes them out again (a leave-one-out baseline).
 *           Integer arithmetic: the words do not depend on how the maps are cut into calls or launches, and adding then
 *           subtracting the same maps restores them exactly.  A subtraction that would take any count below zero sets a flag on
 *           the device and does not fault; p3d_prior_counts and p3d_prior_finish refuse from then on, until p3d_prior_open.
 *           At most P3D_PRIOR_MAX_MAPS maps in all, so that 255 * maps fits a uint32.
 *   FINISH  c_i = (float)count_i, rounded to nearest even (exact below 2^24); then BLUR of the section above with (sigma, radius)
 *           -- RADIUS, TAPS and PASS exactly as there -- then NORM P3D_NORM_MAX.  The result is the handle's prior [H][W], float32,
 *           resident on the device; 1 at the peak.
 *   APPLY   the stage of p3d_set_prior_stage on a map v with the prior g and a weight 0 <= a <= 1, b = (float)(1.0 - (double)a),
 *           float32, no fused multiply-add, every operation rounded once:
 *           P3D_PRIOR_MUL  v' = fmul(v, fadd(fmul(b, g_i), a))      a gain of a where nothing was ever fixated, 1 at the peak;
 *           P3D_PRIOR_MIX  v' = fadd(fmul(b, v), fmul(a, g_i)).
 *           Maps that hold NaN or inf propagate them and are NOT pinned.
 * p3d_prior_open     a zeroed accumulator of H x W counts of `kind` (an open one is replaced; the flag is cleared).  Refused: an
 *                    unknown kind, H * W outside [1, 2^30].
 * p3d_prior_add      maps [n][H][W] of bytes on the host, sign +1 or -1.  Refused on the host before any launch: no accumulator,
 *                    another sign, n < 1, more than P3D_PRIOR_MAX_MAPS maps in all, more maps taken out than are in.
 * p3d_prior_counts   the counts [H][W] and the number of maps (n_maps may be NULL).  Refused: no accumulator, the underflow flag.
 * p3d_prior_info     size, kind and number of maps of the open accumulator; every pointer may be NULL.
 * p3d_prior_finish   FINISH into the handle's prior (the previous one is replaced only on success), and to out [H][W] unless NULL.
 *                    Refused, nothing changed: no accumulator or no maps in it; the underflow flag; every count zero; the blur's
 *                    own refusals (sigma, radius, radius > min(H, W) - 1).
 * p3d_prior_close    frees the accumulator; the finished prior stays.
 * p3d_prior_last_ms  HIP-event times, in ms: [0] the count launches of the last p3d_prior_add, [1] the last p3d_prior_finish's
 *                    launches and the read-back of the maximum.
 * p3d_set_prior_map  a prior [H][W] from the host instead, checked like a baseline: finite and not constant.  NULL drops the
 *                    handle's prior.
 * p3d_get_prior_map  the prior's size (0 x 0 without one) and, unless out is NULL, its H * W floats (cap = room in out, in floats).
 * p3d_set_prior_stage  mode P3D_PRIOR_OFF / P3D_PRIOR_MUL / P3D_PRIOR_MIX and the weight a.  A setting of its own, separate from
 *                    p3d_set_postprocess and p3d_set_hist_match.  The stage sits between BLUR and MATCH of the shared chain:
 *                    resize -> BLUR -> PRIOR -> MATCH -> NORM -> BYTE, in p3d_eval_last_frames (on the scored map, before the
 *                    jitter and every metric), p3d_pred_maps_u8 and p3d_video_maps_u8.  With p3d_set_postprocess off, the two byte
 *                    writers take the float32-resize chain, as they do for MATCH.  Refused: an unknown mode, a outside [0, 1], no
 *                    prior; and, when the stage runs, no prior any more or a prior whose size is not the maps' H x W.
 * p3d_get_prior_stage  the mode and the weight (0 while off); either pointer may be NULL.
 * p3d_set_eval_extra_prior  p3d_set_eval_extra with the handle's prior as the baseline, copied device to device (a later
 *                    p3d_prior_finish does not change it); its minimum, maximum and sum are taken by the same one launch.  flags must
 *                    hold P3D_EVAL_INFO_GAIN.  Refused without a prior; an evaluation of another size than the prior's runs without
 *                    the launch and p3d_last_eval_extra says so, as for a supplied baseline.
 * TEST HOOKS (tests/test_gpu_prior.py); device buffers sit between guard elements, a guard that changed is an error:
 * p3d_debug_prior_count  COUNT of maps [n][H][W] into counts_in [H][W] (NULL: zeros) -> counts_out, flag_out (0 / 1); the maps start
 *                    `offset` (0 .. 3) bytes past a 4-byte boundary.
 * p3d_debug_prior_count_plan  host only: the cut the launcher takes for n maps of H x W at that offset -- four-pixel word lanes,
 *                    one-pixel byte lanes, map slices (more than one: integer atomic adds).
 * p3d_debug_prior_apply  APPLY of maps [n][H][W] against prior [H][W] -> out; the maps start (offset & 3), the prior
 *                    ((offset >> 2) & 3) floats past a 16-byte boundary.
 * p3d_postprocess_maps_prior  p3d_postprocess_maps_match with the stage (prior [H][W]; ignored and may be NULL when mode is off).
 * p3d_debug_eval_maps_prior   p3d_debug_eval_maps_extra with the stage; with P3D_EVAL_INFO_GAIN and a NULL baseline the prior is
 *                    the baseline, copied device to device. */
enum { P3D_PRIOR_FIXATIONS = 0, P3D_PRIOR_BYTES = 1 };
enum { P3D_PRIOR_OFF = 0, P3D_PRIOR_MUL = 1, P3D_PRIOR_MIX = 2 };
#define P3D_PRIOR_MAX_MAPS 16000000
int p3d_prior_open(p3d_handle* h, int H, int W, int kind);
int p3d_prior_add(p3d_handle* h, const unsigned char* maps, int64_t n, int sign);
int p3d_prior_counts(p3d_handle* h, uint32_t* out, int64_t* n_maps);
int p3d_prior_info(p3d_handle* h, int* H, int* W, int* kind, int64_t* n_maps);
int p3d_prior_finish(p3d_handle* h, float sigma, int radius, float* out /* may be NULL */);
int p3d_prior_close(p3d_handle* h);
int p3d_prior_last_ms(p3d_handle* h, double ms[2]);
int p3d_set_prior_map(p3d_handle* h, const float* map, int H, int W);
int p3d_get_prior_map(p3d_handle* h, float* out /* may be NULL */, int64_t cap, int* H, int* W);
int p3d_set_prior_stage(p3d_handle* h, int mode, float a);
int p3d_get_prior_stage(p3d_handle* h, int* mode, float* a);
int p3d_set_eval_extra_prior(p3d_handle* h, int flags);
int p3d_debug_prior_count(int device, int kind, const unsigned char* maps, int64_t n, int H, int W, int sign, const uint32_t* counts_in,
                          int offset, uint32_t* counts_out, int* flag_out);
int p3d_debug_prior_count_plan(int64_t n, int H, int W, int offset, int64_t* words, int64_t* singles, int* slices);
int p3d_debug_prior_apply(int device, int mode, float a, const float* maps, int n, int H, int W, const float* prior, int offset,
                          float* out);
int p3d_postprocess_maps_prior(int device, const float* maps, int n, int h, int w, int elem_stride, int H, int W,
                               const p3d_postprocess* cfg, const p3d_hist_match* match, const float* prior, int mode, float a,
                               float scale, float* out_f32, unsigned char* out_u8);
int p3d_debug_eval_maps_prior(int device, const float* maps, int n_maps, int h, int w, int elem_stride, const unsigned char* density,
                              int Hd, int Wd, const unsigned char* fixation, int H, int W, const double* jitter, const int* borji_idx,
                              const int* n_fix, int n_rep, double step_size, double* out, const p3d_postprocess* cfg,
                              const p3d_hist_match* match, int flags, const float* baseline, double* extra, const float* prior,
                              int mode, float a);

/* ---- Shuffled AUC in the evaluation pass, from a fixation pool on the device (utils/metrics.py:157-197 AUC_shuffled: AUC_Borji
 * whose random locations are fixations of OTHER images, the usual centre-bias-discounting column of video-saliency results; an
 * ADDITION to test.py, which does not call it).  OFF by default: until p3d_eval_shuffled_draws arms an evaluation, every entry point
 * issues exactly the launches it issued before and returns the same bits, and nothing is allocated before p3d_fixpool_open.  The
 * train step, a captured step graph and its schedule never see any of it.  PARITY UNPINNED (the reference's AUC_shuffled takes a
 * ready other_map): this text is the contract, tests/sauc_ref.py replays it in numpy and is itself held to
 * oracle.evaluation.AUC_shuffled; every integer result of the kernels is held to that replay with tolerance 0.
 *   STORE   one pool per handle: words[capacity][nw] of uint64, nw = ceil(H * W / 64), one bit per pixel.  Bit j of word k of a slot
 *           is set exactly when byte 64k + j of its map is >= 128 (the evaluation pass's "fixated" rule); the unused high bits of
 *           the last word are 0.  In numpy: np.packbits(map.ravel() >= 128, bitorder="little"), padded to a multiple of 8 bytes,
 *           viewed as little-endian uint64.  A 1080 x 960 map takes 129 600 bytes.  The host keeps which slots were filled.
 *   UNION   for clip b of a batch and its row ids[b][0 .. M) of filled slots, 1 <= M <= 64 (repeats allowed): uni[b][k] = the OR of
 *           words[ids[b][m]][k]; n_other[b] = the number of set bits; an exclusive uint32 prefix of the words' bit counts, kept in
 *           two levels (within scan blocks of 256 words, and over the blocks).  np.any over the M maps.
 *   SELECT  for a rank 0 <= q < n_other[b]: the pixel index of the q-th set bit of uni[b] in ascending pixel order, an int32:
 *           np.nonzero(other.ravel())[0][q], exactly.
 *   DRAW ORDER  the host draws; the device never does.  Python's metrics.shuffled_draws is the one place: per clip in clip order,
 *           nothing for a clip with n_fix = 0, else for each of the n_rep splits in order rng.permutation(n_other_b)[:n_fix_b];
 *           clip b's ranks are the transposed rows [min(n_fix_b, n_other_b)][n_rep], row-major, clips concatenated.  A driver that
 *           also draws the other clips from the same stream draws all rows of ids for the batch first (clip order), calls
 *           p3d_eval_shuffled_begin, then draws the permutations (clip order): drivers/test.py --sauc-device.
 *   SCORE   the armed p3d_eval_last_frames, after all its launches (unedited, in their order): SELECT of every rank; then pass A and
 *           pass B of the evaluation (p3d_full_moments) on the CLEAN scored map P -- after the resize and the optional BLUR / PRIOR /
 *           MATCH / NORM stages, WITHOUT AUC_Judd's jitter (with P3D_MATCH_DENSITY that is the map matched to its own density) --
 *           with statistics and scratch of their own; then the AUC_Borji kernel with clip b's n_rows[b] rows of selected pixels.
 *           The false-positive rate divides by n_fix also when n_other < n_fix (utils/metrics.py:151-152); with n_other = 0 the
 *           curve closes at (1, 1); a clip without fixation gives NaN for every split.  These are the launches and inputs of
 *           p3d_metric_auc_shuffled on that map: the same bits.  The mean over the splits is the host's (np.mean).  out[B][5], KL
 *           and IG are bit for bit what they are unarmed.
 * p3d_fixpool_open   a pool of `capacity` slots for maps of H x W bytes (an open one is replaced, with the union held for it).
 *                    Refused: H * W outside [1, 2^30], capacity outside [1, 2^31 - 1].
 * p3d_fixpool_put    maps [n][H][W] of bytes on the host into slots first .. first + n - 1, through a staging buffer of at most
 *                    256 MB.  Refused before any launch: no pool, n < 1, a slot outside [0, capacity).
 * p3d_fixpool_info   size, capacity, words per map and number of filled slots; every pointer may be NULL.
 * p3d_fixpool_get    the words [n][nw] of filled slots first .. first + n - 1 (for tests).  Refused: an unfilled slot, a slot outside.
 * p3d_fixpool_close  frees the pool, its staging buffer and the union.
 * p3d_fixpool_last_ms  HIP-event times, in ms: [0] the pack launches of the last p3d_fixpool_put, [1] the union + scan launch of the
 *                    last p3d_eval_shuffled_begin, [2] the select and [3] the clean moments + borji of the last armed evaluation.
 * p3d_eval_shuffled_begin  UNION for the handle's batch: ids [B][M] on the host, checked row by row before any launch (every id a
 *                    filled slot, 1 <= M <= 64); n_other_out[B] comes back after one synchronisation; the union and its scan stay
 *                    in buffers of the handle.  Independent of the prediction: before or after the forward pass.  Disarms.
 * p3d_eval_shuffled_draws  the host's ranks, [n_rows[b]][n_rep] per clip, concatenated, and the threshold step of the curve.  Refused
 *                    before anything is kept: no union held, n_rows[b] > n_other[b], a rank outside [0, n_other[b]), n_rep < 1, a
 *                    step that is not positive.  Arms exactly ONE evaluation: the next p3d_eval_last_frames, whatever becomes of it.
 *                    That evaluation refuses, before any launch, a pool of another size than its H x W, a batch of another size
 *                    than the union's, and n_rows[b] != min(n_fix[b], n_other[b]) (n_fix itself is held to the device's count
 *                    as always).
 * p3d_last_eval_shuffled  per_rep[B][n_rep] of the last armed evaluation that succeeded (cap = room in doubles).  An evaluation
 *                    that was not armed clears nothing and adds nothing.
 * TEST HOOKS (tests/test_gpu_sauc_device.py); device buffers sit between guard elements, a guard that changed is an error:
 * p3d_debug_fix_pack     STORE of maps [n][H][W] -> words [n][nw]; the maps start `offset` (0 .. 3) bytes past a 16-byte boundary.
 * p3d_debug_fix_union    UNION over a pool of packed words [capacity][nw] -> uni [B][nw], the exclusive prefix over the whole map
 *                    [B][nw] (block sum + block-local prefix; may be NULL), n_other [B].
 * p3d_debug_fix_select   UNION, then SELECT of ranks ([n_rows[b]][n_rep] per row, concatenated) -> out, int32, the same layout.
 * p3d_debug_eval_maps_shuffled  p3d_debug_eval_maps_prior (a supplied baseline only) with the whole armed sequence on caller-supplied
 *                    maps: pool_maps [capacity][H][W] are packed, the union taken, n_other [B] returned, and the evaluation scored
 *                    with the given ranks -> per_rep [n_maps][sh_n_rep]. */
#define P3D_FIX_SCAN_BLOCK 256
int p3d_fixpool_open(p3d_handle* h, int H, int W, int64_t capacity);
int p3d_fixpool_put(p3d_handle* h, int64_t first, const unsigned char* maps, int64_t n);
int p3d_fixpool_info(p3d_handle* h, int* H, int* W, int64_t* capacity, int64_t* words_per_map, int64_t* n_filled);
int p3d_fixpool_get(p3d_handle* h, int64_t first, int64_t n, uint64_t* words);
int p3d_fixpool_close(p3d_handle* h);
int p3d_fixpool_last_ms(p3d_handle* h, double ms[4]);
int p3d_eval_shuffled_begin(p3d_handle* h, const int* ids, int M, uint32_t* n_other_out);
int p3d_eval_shuffled_draws(p3d_handle* h, const int* ranks, const int* n_rows, int n_rep, double step);
int p3d_last_eval_shuffled(p3d_handle* h, double* per_rep, int64_t cap);
int p3d_debug_fix_pack(int device, const unsigned char* maps, int n, int H, int W, int offset, uint64_t* words);
int p3d_debug_fix_union(int device, const uint64_t* pool, int capacity, int H, int W, const int* ids, int B, int M, uint64_t* uni,
                        uint32_t* prefix /* may be NULL */, uint32_t* n_other);
int p3d_debug_fix_select(int device, const uint64_t* pool, int capacity, int H, int W, const int* ids, int B, int M, const int* ranks,
                         const int* n_rows, int n_rep, int* out);
int p3d_debug_eval_maps_shuffled(int device, const float* maps, int n_maps, int h, int w, int elem_stride, const unsigned char* density,
                                 int Hd, int Wd, const unsigned char* fixation, int H, int W, const double* jitter, const int* borji_idx,
                                 const int* n_fix, int n_rep, double step_size, double* out, const p3d_postprocess* cfg,
                                 const p3d_hist_match* match, int flags, const float* baseline, double* extra, const float* prior,
                                 int mode, float a, const unsigned char* pool_maps, int capacity, const int* ids, int M,
                                 const int* ranks, const int* n_rows, int sh_n_rep, double sh_step, uint32_t* n_other, double* per_rep);

/* ---- Resident video inference (an ADDITION beside p3d_predict_windows: gen_pred.py slides a 16-frame queue by one frame and keeps
 * nothing on the device).  A video's normalised frames go up once, windows are cut where the frames are, and every frame's map is
 * kept on the device until it is read.  OFF until p3d_video_open: while no video is open every other entry point issues what it
 * issued before and returns the same bits, and nothing is allocated.  Open and close do not drop a captured step graph; the staged
 * input keeps its address and is only overwritten, as p3d_upload_inputs overwrites it.  Works under p3d_ema_swap as
 * p3d_predict_windows does; with world_size > 1 it is local to the rank.  PARITY: P3D_VIDEO_NEWEST with starts 0, 1, 2, ... is the
 * reference's rule (gen_pred.py:154-168: the first window writes all T maps, every later one its newest frame).  Other strides and
 * P3D_VIDEO_MEAN are UNPINNED: this text is their contract and tests/video_ref.py replays it in numpy bit for bit.
 * T, H, W, B below are the handle's frames, height, width and batch; F the open video's frames.
 *
 * p3d_video_open   allocates, on the handle's device, a frame store [F][H][W][3] float32, a map store [F][H][W] float32 and a
 *                  contribution count per frame, all 0; no frame counts as put and last_start = -1.  Opening again replaces the
 *                  video; the allocation is reused when it is large enough.  Refused (-1, nothing changed): frames < T, a mode that
 *                  is neither of the two, a store the device cannot hold.
 * p3d_video_close  frees the stores.  p3d_video_info: F, the mode and the last start accepted since the open (-1: none); any pointer
 *                  may be NULL; refused while no video is open, like every call below.
 * p3d_video_put_frames     copies n normalised frames x [n][H][W][3] to frames first .. first + n - 1.
 * p3d_video_put_frames_u8  uploads n decoded frames bgr [n][H0][W0][3] and normalises them straight into the store: the stored
 *                  floats are, bit for bit, what p3d_mapf_frames returns for those frames.  Frames may arrive in any order and in
 *                  several calls; a range outside [0, F) is refused.  (p3d_video_keep_source, "Rendering 8-bit maps" below, also
 *                  keeps the bytes; off, this call issues what it always issued.)
 * p3d_video_predict  n_windows in 1 .. B; starts strictly ascending, every start greater than last_start and inside [0, F - T], and
 *                  every frame of every window put.  Anything else: -1, p3d_last_error names the first offending window or
 *                  frame, nothing is launched and nothing changes.  Then:
 *     GATHER   one launch: clip k of the staged input = frames starts[k] .. starts[k] + T - 1 of the store, a copy of the bits.
 *              Clips n_windows .. B - 1 are copies of the last window (they keep the per-clip BatchNorm statistics finite and
 *              contribute nothing below).
 *     FORWARD  p3d_predict_windows's pass (per-clip statistics, not training, no dropout): the prediction of clip k equals, bit
 *              for bit, what p3d_predict_windows returns for clip k on the same windows stacked and padded by the host.
 *              p3d_pred_maps_u8 keeps working on the batch.
 *     SCATTER  one launch, no atomics.  For k ascending and t = 0 .. T - 1, with f = starts[k] + t:
 *              P3D_VIDEO_NEWEST  if count[f] == 0: map[f] = pred[k][t], a copy of the bits, and count[f] = 1; else frame f is left
 *                                alone (every frame comes from the first window that holds it);
 *              P3D_VIDEO_MEAN    if count[f] == 0: sum[f] = pred[k][t], a copy of the bits (-0 stays -0); else
 *                                sum[f] = fadd(sum[f], pred[k][t]) in float32; then count[f] += 1.  The ascending rule fixes the
 *                                order ((p_s0 + p_s1) + p_s2) + ..., so the bits do not depend on the run or the batching.
 *     last_start = starts[n_windows - 1].  The call returns synchronised.
 * p3d_video_get_maps  frames first .. first + n - 1 -> maps [n][H][W]: the stored map under NEWEST; under MEAN
 *                  __fdiv_rn(sum, (float)count) per element (a count of 1 returns the sum's bits), computed into scratch: the sums
 *                  are not rewritten, so more windows can follow.  counts (or NULL) [n] receives the frames' counts.  A frame
 *                  with count 0 is refused and the error names it.
 * p3d_video_maps_u8   p3d_pred_maps_u8's chain on those maps (MEAN: finalised into scratch first) -> out [n][H][W] bytes: the
 *                  double-precision p3d_resize_linear_u8 law, or under p3d_set_postprocess the float32 resize / BLUR / NORM / BYTE
 *                  sequence, 16 maps at a time.  stage_ms as p3d_pred_maps_u8's.
 * p3d_video_last_ms   HIP-event time of the last p3d_video_predict's gather (ms[0]) and scatter (ms[1]) launches, milliseconds. */
enum { P3D_VIDEO_NEWEST = 0, P3D_VIDEO_MEAN = 1 };
int p3d_video_open(p3d_handle* h, int frames, int mode);
int p3d_video_close(p3d_handle* h);
int p3d_video_info(p3d_handle* h, int* frames, int* mode, int* last_start);
int p3d_video_put_frames(p3d_handle* h, int first, const float* x, int n);
int p3d_video_put_frames_u8(p3d_handle* h, int first, const unsigned char* bgr, int n, int H0, int W0, const float mean_rgb[3]);
int p3d_video_predict(p3d_handle* h, const int* starts, int n_windows);
int p3d_video_get_maps(p3d_handle* h, int first, int n, float* maps, int32_t* counts /* may be NULL */);
int p3d_video_maps_u8(p3d_handle* h, int first, int n, float scale, int H, int W, unsigned char* out, double* stage_ms);
int p3d_video_last_ms(p3d_handle* h, double ms[2]);
/* Test hooks: the three launches from the launch descriptions the entry points use, on host arrays.  Every device buffer sits
 * `offset` (0 .. 3) elements past a 16-byte boundary between guard elements; -1 if a guard or an input changed.
 *   gather   store [F][frame_elems], starts [n_windows] each in [0, F - T] -> x [B][T][frame_elems] (padded as GATHER above);
 *   scatter  pred [B][T][hw][ld] (channel 0 is the map), validated as p3d_video_predict validates (every frame counts as put);
 *            store [F][hw] and count [F] are updated in place, and the counts the device wrote must equal the plan's;
 *   mean     sum [n][hw], count [n] (each >= 1) -> out [n][hw];
 *   plan     host only, no HIP call: validates as p3d_video_predict does and returns the counts after the call in count_out [F]
 *            (untouched after a refusal). */
int p3d_debug_video_gather(int device, const float* store, int F, int T, int64_t frame_elems, const int* starts, int n_windows, int B,
                           int offset, float* x);
int p3d_debug_video_scatter(int device, int mode, const float* pred, int B, int T, int64_t hw, int ld, const int* starts, int n_windows,
                            int F, int last_start, float* store /* in/out [F][hw] */, int32_t* count /* in/out [F] */, int offset);
int p3d_debug_video_mean(int device, const float* sum, const int32_t* count, int n, int64_t hw, int offset, float* out);
int p3d_debug_video_plan(int mode, int F, int T, int B, int last_start, const int32_t* count_in, const int* starts, int n_windows,
                         int32_t* count_out);

/* ---- Temporal smoothing of the open video's maps at read-out (an ADDITION: overlapping 16-frame windows flicker from frame to
 * frame, and every other output stage works on one map in space).  OFF by default; off, every entry point issues what it issued
 * before and returns the same bits.  Nothing is allocated until the stage first runs (scratch from the stream pool); the train
 * step, a captured step graph and its schedule never see it.  PARITY UNPINNED: the reference has no such stage, so this text is
 * the contract and tests/temporal_ref.py replays it in numpy bit for bit.  The stage filters along the frame axis into scratch:
 * the stores are never rewritten, so more windows can follow a filtered read.  One launch per read-out call.
 *   INPUT   v_f, the input of frame f, per element: under P3D_VIDEO_NEWEST the stored map; under P3D_VIDEO_MEAN
 *           __fdiv_rn(sum_f, (float)count_f), a count of 1 giving the sum's bits: what p3d_video_get_maps returns with the stage
 *           off.  The division happens as the temporal kernel loads the frame; no finalised copy of the video is written.
 *   GAUSS   P3D_TEMPORAL_GAUSS: radius and taps follow RADIUS and TAPS of the postprocess section (p3d_blur_taps(sigma, radius)),
 *           with sigma > 0, the resulting r in 1 .. P3D_TEMPORAL_MAX_RADIUS, and r <= F - 1.  The output is that section's PASS
 *           along the frame axis of the WHOLE video (n = F): float32, no fused multiply-add, reflect-101 at frames 0 and F - 1:
 *           acc = fmul(w_r, v_f);  for d = 1 .. r:  acc = fadd(acc, fmul(w_{r+d}, fadd(v_{rho(f-d)}, v_{rho(f+d)}))).
 *           fadd commutes, so the filter commutes bit for bit with reversing the video in time.  A read of frames
 *           first .. first + n - 1 needs frames max(0, first - r) .. min(F - 1, first + n - 1 + r).
 *   EMA     P3D_TEMPORAL_EMA (causal): alpha finite and in [0, 1);  b = fsub(1.0f, alpha);  m_0 = v_0, a copy of the bits;
 *           m_f = fadd(fmul(alpha, m_{f-1}), fmul(b, v_f));  the output of frame f is m_f.  A read of first .. first + n - 1 needs
 *           frames 0 .. first + n - 1 and recomputes from frame 0 in every call (no carry is kept): the bits of a partial read
 *           are the slice of a full read.
 * Maps that hold NaN or inf propagate them; their results are NOT pinned.
 * Refused (-1, p3d_last_error set, nothing launched, nothing changed) at set time: an unknown kind; GAUSS with sigma not finite or
 * not > 0, radius < 0 or > P3D_TEMPORAL_MAX_RADIUS (also the radius that follows from sigma), or a resulting r of 0; EMA with alpha
 * not finite or outside [0, 1).  (sigma and radius are not read under EMA, alpha not under GAUSS.)  At read-out time: r > F - 1; a
 * needed frame whose count is 0 -- the error names the first such frame.
 *
 * p3d_set_video_temporal  the handle's setting; NULL or kind P3D_TEMPORAL_OFF switch it off; needs no open video and outlives it.
 * p3d_get_video_temporal  the setting (zeros while off) and whether it is on; either pointer may be NULL.
 * While on:
 *   p3d_video_get_maps  returns the filtered maps; counts are the frames' own counts, as before.
 *   p3d_video_maps_u8   filters first, then its chain runs on the filtered maps, 16 at a time: the double-precision
 *                       p3d_resize_linear_u8 law, or under p3d_set_postprocess / p3d_set_hist_match / p3d_set_prior_stage the
 *                       float32 resize, BLUR, prior, match, NORM, BYTE.
 * p3d_video_temporal_last_ms  HIP-event time of the temporal launch of the last read-out that ran the stage, milliseconds.
 * p3d_temporal_filter  the stage alone on host maps [F][hw] (every count 1) -> out [n][hw], frames first .. first + n - 1.
 * Test hooks.  p3d_debug_video_temporal: the launch from the launch description the read-outs use, on a host store [F][hw] and
 * counts [F] under `mode`; every device buffer sits `offset` (0 .. 3) elements past a 16-byte boundary between guard elements;
 * -1 if a guard, the store or the counts changed.  Its refusals are decided before the first HIP call.
 * p3d_debug_video_temporal_plan (host only, no HIP call): for GAUSS of radius r on hw pixels and a read of n frames, the pixels and
 * the consecutive output frames one block owns (block (x, y) takes pixels from x * pixels_per_block and frames from
 * first + y * frames_per_block) and its LDS bytes, at most 65536; for EMA (r is not read) the pixels of one block with 16-byte
 * aligned bases, n, and 0.
 * p3d_debug_video_temporal_desc (host only): the launch description of a read-out of frames first .. first + n - 1 of F frames of
 * hw pixels under `mode` -- the kernel's name (cap = room in kernel, in bytes), and the float operations and the bytes it claims:
 * every input frame once per block run that loads it, every output frame once. */
enum { P3D_TEMPORAL_OFF = 0, P3D_TEMPORAL_GAUSS = 1, P3D_TEMPORAL_EMA = 2 };
#define P3D_TEMPORAL_MAX_RADIUS 24
typedef struct p3d_video_temporal { int kind; float sigma; int radius; float alpha; } p3d_video_temporal;
int p3d_set_video_temporal(p3d_handle* h, const p3d_video_temporal* cfg);
int p3d_get_video_temporal(p3d_handle* h, p3d_video_temporal* cfg, int* on);
int p3d_video_temporal_last_ms(p3d_handle* h, double* ms);
int p3d_temporal_filter(int device, const p3d_video_temporal* cfg, const float* maps, int F, int64_t hw, int first, int n, float* out);
int p3d_debug_video_temporal(int device, int mode, const p3d_video_temporal* cfg, const float* store, const int32_t* count, int F,
                             int64_t hw, int first, int n, int offset, float* out);
int p3d_debug_video_temporal_plan(int kind, int r, int64_t hw, int n, int* pixels_per_block, int* frames_per_block, int* lds_bytes);
int p3d_debug_video_temporal_desc(int mode, const p3d_video_temporal* cfg, int F, int64_t hw, int first, int n, char* kernel, int cap,
                                  double* flops, double* bytes);

/* ---- Resident training set (an ADDITION beside p3d_upload_inputs: the reference's loader, dataflow.py:39-62, cuts clips that
 * share overlap of video_length frames on the host and keeps nothing on the device).  The decoded frames, density maps and fixation
 * maps of V videos go up once; a batch of B clips, each a (video, start) pair, is cut where they are, into the staged x, y and
 * fixation buffers a train step reads, normalising on the way.  OFF until p3d_trainset_open: while no set is open every other entry
 * point issues what it issued before and returns the same bits, and nothing is allocated.  No step, launch list or captured graph
 * names the stores, a captured step graph survives every call here, checkpoints store nothing of the set, a resident video and a
 * training set may be open together, and with world_size > 1 the set is local to the rank.
 * T, H, W, B below are the handle's frames, height, width and batch; F_v is video v's frames; the videos are concatenated, video v's
 * frames at base[v] = F_0 + .. + F_{v-1}.
 *
 * STORES (tests/trainset_ref.py replays every rule below in numpy bit for bit):
 *   frames     one format per set.  P3D_TRAINSET_FRAMES_U8: 3 bytes per grid pixel, the decoded bytes as put; takes only frames decoded
 *              at H x W.  P3D_TRAINSET_FRAMES_F32: the floats p3d_mapf_frames returns, for any source size.
 *   density    one byte per grid pixel: the byte v of p3d_mapf_density's 8-bit resize (a copy when the sizes agree), y = v / 255.
 *   fixations  one byte per grid pixel; exists only in a set opened with P3D_TRAINSET_FIXATIONS.
 *   and a put flag per frame and tensor, on the host.
 *
 * p3d_trainset_open   allocates the stores for n_videos videos of frames[v] >= 1 frames each on the handle's device and clears every
 *                     put flag.  mean_rgb: the channel means every frame is normalised with.  Opening again replaces the set; an
 *                     allocation that is large enough is reused.  Refused (-1, nothing changed): no video, a video without frames,
 *                     more than 2^31 - 1 frames, an unknown format or flag, a mean that is not finite, no device memory.
 * p3d_trainset_close  frees the stores.
 * p3d_trainset_info   V, the frames of all videos, the format, the flags and the bytes of the stores; any pointer may be NULL; refused
 *                     while no set is open, like every call below.  p3d_trainset_video_info: F_v and how many of its frames were put,
 *                     per tensor.
 * p3d_trainset_put_frames_u8   n decoded frames bgr [n][H0][W0][3] (cv2's order) -> frames first .. first + n - 1 of `video`.  U8 sets
 *                     keep the bytes (H0 x W0 must be H x W); F32 sets keep p3d_mapf_frames(bgr, H0, W0, mean_rgb, H, W).
 * p3d_trainset_put_frames      F32 sets only: n normalised frames x [n][H][W][3], a copy.
 * p3d_trainset_put_density_u8  n grey maps [n][H0][W0] -> the bytes of p3d_mapf_density's resize to H x W.
 * p3d_trainset_put_fixations   n maps [n][H][W] on the grid, a copy of the bytes (fixated where >= 128, as p3d_upload_fixations).
 *                     A put outside its video, or one the set's format or flags exclude, is refused with nothing changed.
 * p3d_trainset_stage  clip k = frames start[k] .. start[k] + T - 1 of video[k], k < n == B:
 *                       staged x   = p3d_mapf_frames of the clip's frames, bit for bit (U8 sets, per channel c of RGB:
 *                                    __fdiv_rn(__fsub_rn((float)bgr[2 - c], mean_rgb[c]), 255.f), which is that kernel at equal sizes)
 *                       staged y   = p3d_mapf_density of the clip's maps: (float)((double)v / 255.0)
 *                       staged fixations = the bytes, exactly when the set has them; that counts as the p3d_upload_fixations
 *                                    p3d_train_step_device asks for, and allocates that buffer on first use as the first upload does.
 *                     Validated first: n == B, every video in [0, V), every start in [0, F_v - T], every frame of every clip put in
 *                     every tensor the call writes.  Else -1, p3d_last_error names the first offending clip or frame, nothing is
 *                     launched and nothing changes.  One launch; the staged buffers keep their addresses; returns synchronised.  Each
 *                     call overwrites the staged input, as p3d_upload_inputs does.
 * p3d_trainset_step   p3d_trainset_stage, p3d_augment_inputs(seed) under p3d_set_augment, p3d_train_step_device(dropout, seed),
 *                     p3d_last_loss: the loss and every weight, slot, moving statistic and shadow equal those after p3d_train_step (with
 *                     p3d_upload_fixations where the loss reads them) on host clips built through p3d_mapf_frames / p3d_mapf_density.
 *                     Under p3d_set_grad_accum each call is one micro-step.  Refused with nothing changed when the loss reads fixations
 *                     (P3D_LOSS_SALIENCY with w_nss > 0) and the set has none, and wherever the stage or p3d_train_step refuses.
 * p3d_trainset_forward  stages x only (density and fixations need not be put), then p3d_forward's pass with training off and
 *                     dropout 0 -> pred, as p3d_forward returns it for the host-built clips.
 * p3d_trainset_get_staged  reads the staged buffers back: x [B][T][H][W][3], y [B][T][H][W], fix [B][T][H][W]; any may be NULL.
 * p3d_trainset_last_ms  HIP-event time of the last stage's launch (p3d_trainset_stage / _step / _forward), milliseconds.
 *
 * Test hook.  p3d_debug_trainset_gather: the launch from the launch description the handle uses, on host stores of n_videos videos
 * (frames_store: bytes for format U8, floats for F32; density_store / fix_store [sum F][hw] bytes, either may be NULL with its
 * output) -> x [B][T][hw][3], y, fix.  Every device buffer sits `offset` (0 .. 3) elements past a 16-byte boundary between guard
 * elements; -1 if a guard or a store changed, or if the launch wrapper refused the table (a row outside its video).  first: NULL,
 * or the rows' first frames in the concatenation as the caller computed them (the wrapper refuses a row that is not
 * base[video] + start). */
enum { P3D_TRAINSET_FRAMES_U8 = 0, P3D_TRAINSET_FRAMES_F32 = 1 };
#define P3D_TRAINSET_FIXATIONS 1
int p3d_trainset_open(p3d_handle* h, int n_videos, const int* frames, int frame_format, int flags, const float mean_rgb[3]);
int p3d_trainset_close(p3d_handle* h);
int p3d_trainset_info(p3d_handle* h, int* n_videos, int64_t* total_frames, int* frame_format, int* flags, int64_t* bytes);
int p3d_trainset_video_info(p3d_handle* h, int video, int* frames, int* put_frames, int* put_density, int* put_fixations);
int p3d_trainset_put_frames_u8(p3d_handle* h, int video, int first, const unsigned char* bgr, int n, int H0, int W0);
int p3d_trainset_put_frames(p3d_handle* h, int video, int first, const float* x, int n);
int p3d_trainset_put_density_u8(p3d_handle* h, int video, int first, const unsigned char* grey, int n, int H0, int W0);
int p3d_trainset_put_fixations(p3d_handle* h, int video, int first, const unsigned char* fix, int n);
int p3d_trainset_stage(p3d_handle* h, const int* video, const int* start, int n);
int p3d_trainset_step(p3d_handle* h, const int* video, const int* start, int n, float dropout_rate, uint64_t seed, float* loss);
int p3d_trainset_forward(p3d_handle* h, const int* video, const int* start, int n, float* pred);
int p3d_trainset_get_staged(p3d_handle* h, float* x, float* y, unsigned char* fix);
int p3d_trainset_last_ms(p3d_handle* h, double* ms);
int p3d_debug_trainset_gather(int device, int frame_format, const void* frames_store, const unsigned char* density_store,
                              const unsigned char* fix_store, int n_videos, const int* frames, int T, int64_t hw, const float mean_rgb[3],
                              const int* video, const int* start, const int* first, int B, int offset, float* x, float* y,
                              unsigned char* fix);

/* ---- Scoring 8-bit maps against 8-bit ground truth (an ADDITION: the arithmetic of the reference's
 * utils/matlab_metric/metric_video_base.m protocol -- every frame's 8-bit map at output resolution against that frame's 8-bit density
 * and fixation images, CC / SIM / AUC-Judd per frame with KL and NSS behind masks -- with the metric definitions of
 * utils/metrics.py; the MATLAB toolbox and metric_statistics are not part of this library).  OFF until called: every other entry
 * point issues what it issued before and returns the same bits.  PARITY UNPINNED beyond utils/metrics.py: this text is the
 * contract, tests/score_u8_ref.py replays it in numpy and is itself held to oracle/metrics.py.
 * Per map: saliency s, density d, fixation x, [H][W] bytes of one shape, N = H * W, 1 <= N <= 2^23 (every integer below then fits
 * a signed 64-bit word: 65025 * 2^46 < 2^63).  A pixel is fixated exactly when its byte x >= 128.
 *   TABLES  hs[v] = pixels with s = v; hf[v] = fixated pixels with s = v; hd[v] = pixels with d = v; sd = sum s d (uint64).
 *           Integers: no order can show.  From them, exactly: S1 = sum v hs[v], S2 = sum v^2 hs[v], D1, D2 likewise from hd,
 *           nf = sum hf[v], F1 = sum v hf[v].
 *   Everything below is float64, every operation rounded on its own; (double) of an integer is one round-to-nearest-even.
 *   CC      (double)(N sd - S1 D1) / (sqrt((double)(N S2 - S1^2)) * sqrt((double)(N D2 - D1^2))), the three differences formed as
 *           integers; NaN when either variance is 0.
 *   NSS     (double)(N F1 - nf S1) / ((double)nf * sqrt((double)(N S2 - S1^2))); NaN when nf = 0 or the variance is 0.
 *   AUC_Judd, P3D_SCORE_TIES_REFERENCE  utils/metrics.py:69-85 with jitter=False: walk v = 255 .. 0 with A += hs[v]; for each of
 *           the hf[v] fixations of that level k += 1 and the point tp = k / nf, fp = (A - k) / (N - nf) is added; with the end
 *           points (0, 0) and (1, 1) the score is sum (fp_i+1 - fp_i) (tp_i+1 + tp_i) / 2.  Inside a tied level fp runs backwards;
 *           that is the reference's behaviour.  With G_v = sum_{u > v} hf[u] the sum times 2 (N - nf) nf is the integer
 *           I = sum_v hs[v] w_v - nf^2, w_v = 2 G_v + 1 where G_v < nf and 2 nf where G_v = nf, and the score is
 *           (double)I / (double)(2 (N - nf) nf): the sweep's real value, rounded once.
 *   AUC_Judd, P3D_SCORE_TIES_EXPECTED  the expectation of that curve's score when the pixels inside every level are ordered
 *           uniformly at random -- what the reference's default jitter does to an 8-bit map, without a draw.  m[v] = hs[v] - hf[v],
 *           f = (double)hf[v], g = (double)G_v, n = (double)nf:
 *             e_v = ((g + 0.5) + f / 2) / n                                          where G_v + hf[v] < nf,
 *             e_v = (((f * (g + 0.5)) / n + (f * (f - 1)) / (2 n)) + 1) / (f + 1)   where G_v + hf[v] = nf;
 *           t_v = (double)m[v] * e_v, and 0 where m[v] = 0; score = T / (double)(N - nf), T the sum of t_255 .. t_0 in this order:
 *           with t_255 first, groups of 64 consecutive terms are each folded by six butterfly steps (x_i += x_{i xor o}, o = 32,
 *           16, 8, 4, 2, 1), then T = ((w0 + w1) + w2) + w3.
 *           Both laws: NaN when nf = 0, and NaN when nf = N (the reference divides by zero there: not pinned).
 *   SIM     min_s / max_s the lowest / highest v with hs[v] > 0; u_v = (double)(v - min_s) / (double)(max_s - min_s);
 *           U_s = sum over v ascending, hs[v] > 0 only, of (double)hs[v] * u_v; us[v] = u_v / U_s; ud from hd likewise.
 *           SIM = sum over pixels of min(us[s], ud[d]), a NaN on either side kept (a constant map gives NaN).
 *   KL      ps[v] = (double)v / (double)S1, or 0 for every v when S1 = 0 (the reference's `if map1.any()`); pd from D1 likewise;
 *           KL = sum over pixels of pd[d] * log(eps + pd[d] / (ps[s] + eps)), eps = 2.2204e-16 (utils/metrics.py:359, the literal).
 *           The imresize of the reference's KLdiv is the identity on maps of one shape and its byte quantisation is not reproduced.
 *           The order of the two sums over pixels is the kernel's (lane, then block partials in block order); tests hold them
 *           to relative 1e-9.
 * p3d_video_score    scores frames first .. first + n - 1 of the open video.  The scored bytes are, bit for bit, what
 *                    p3d_video_maps_u8(first, n, scale, H, W) returns under the handle's current settings (MEAN finalisation,
 *                    p3d_set_video_temporal, p3d_set_postprocess, p3d_set_prior_stage, P3D_MATCH_TABLE); they stay on the device
 *                    unless maps_out asks for them.  density / fixation [n][H][W] on the host; out [n][5]: CC, SIM, AUC_Judd, KL,
 *                    NSS, an unselected column NaN.  stage_ms (or NULL) [3]: HIP-event milliseconds of the two uploads, of the
 *                    maps' chain, of the scoring launches.  Validated as p3d_video_maps_u8 validates, before any launch or
 *                    upload; also refused: flags outside the five bits or 0, a ties law that is neither value, H * W > 2^23,
 *                    fixation == NULL with JUDD or NSS selected (without them it may be NULL).
 * p3d_score_maps_u8  op level, host arrays: n maps sal / density / fixation [n][H][W] -> out [n][5]; n in 1 .. 65535.
 * TEST HOOKS (tests/test_gpu_score_u8.py):
 * p3d_debug_score_u8   the same launch descriptions with every device buffer between guard elements: sal starts `offset` bytes
 *                    (0 .. 15) past a 16-byte boundary, density (2 offset) mod 16 and fixation (3 offset) mod 16 bytes past one, so
 *                    that offset 0 aligns the three alike and any other offset does not; -1 if a guard or an input changed, or if
 *                    anything was written for pass B when neither SIM nor KL was selected.  hs / hf / hd [n][256] and sd [n] come
 *                    back; any of the four may be NULL.
 * p3d_debug_score_plan host only, no HIP call: pass A's blocks per map, pixels per block (a multiple of 16) and the most products
 *                    s d a lane adds in its 32-bit accumulator for n maps at that offset (66 051 products of 255 * 255 fit). */
enum { P3D_SCORE_CC = 1, P3D_SCORE_SIM = 2, P3D_SCORE_JUDD = 4, P3D_SCORE_KL = 8, P3D_SCORE_NSS = 16 };
#define P3D_SCORE_MATLAB (P3D_SCORE_CC | P3D_SCORE_SIM | P3D_SCORE_JUDD)      /* metric_video_base.m's masks */
enum { P3D_SCORE_TIES_REFERENCE = 0, P3D_SCORE_TIES_EXPECTED = 1 };
int p3d_video_score(p3d_handle* h, int first, int n, float scale, int H, int W, const unsigned char* density,
                    const unsigned char* fixation, int flags, int ties, double* out, unsigned char* maps_out /* may be NULL */,
                    double* stage_ms /* may be NULL */);
int p3d_score_maps_u8(int device, const unsigned char* sal, const unsigned char* density, const unsigned char* fixation, int n, int H,
                      int W, int flags, int ties, double* out);
int p3d_debug_score_u8(int device, const unsigned char* sal, const unsigned char* density, const unsigned char* fixation, int n, int H,
                       int W, int flags, int ties, int offset, uint32_t* hs, uint32_t* hf, uint32_t* hd, uint64_t* sd, double* out);
int p3d_debug_score_plan(int64_t n_pix, int n, int offset, int* blocks_per_map, int* pixels_per_block, int64_t* products_per_lane);

/* ---- AUC-Borji and shuffled AUC of 8-bit maps (an ADDITION: metric_video_base.m's saliency_score_BOR column, lines 132-135, and
 * the shuffled AUC that video-saliency tables report beside it, with the definitions of utils/metrics.py:88-197).  OFF until called:
 * every other entry point issues what it issued before and returns the same bits.  PARITY UNPINNED beyond utils/metrics.py: this
 * text is the contract, tests/score_auc_ref.py replays it in numpy and is itself held to oracle.metrics.AUC_Borji and
 * oracle.evaluation.AUC_shuffled (per split, absolute 1e-12: np.trapz adds the same terms in its own order).
 *   SPLIT SWEEP  Per map: saliency bytes s and fixation bytes x, [H][W] each, N = H * W, 1 <= N <= 2^23; a pixel is fixated exactly
 *           when x >= 128.  Sample pixel indices idx[n_rows][n_rep], int32, row-major (the reference's [n_fix, n_rep]).
 *           hs, hf, nf as in TABLES above; lo / hi the lowest / highest v with hs[v] > 0; maxfix the highest v with hf[v] > 0
 *           (-1 when nf = 0); u_v = (double)(v - lo) / (double)(hi - lo); kmax = (int)ceil(1.0 / step), a step that is not
 *           positive or gives kmax > 1024 is refused; t_k = (double)k * step; lev[v] = the number of k < kmax with t_k <= u_v,
 *           for every v in 0 .. 255 (0 for every v on a flat map, hi = lo).
 *           For split rep: b_i = s[idx[i][rep]]; top = max(maxfix, max_i b_i) (n_rows = 0: maxfix); K = (int)ceil(u_top / step),
 *           or 0 when u_top = 0 -- len(np.arange(0, u_top, step)).  For k = K - 1 .. 0, in this order: ctp = sum of hf[v] over
 *           lev[v] > k; cfp = the number of i with lev[b_i] > k (both integers); x = (double)cfp / (double)nf,
 *           y = (double)ctp / (double)nf; area += (x - px) * (y + py) * 0.5, from (px, py) = (0, 0); then (px, py) = (x, y).  After
 *           the last k the closing term (1 - px) * (1 + py) * 0.5 is added.  float64, every operation rounded on its own.  The
 *           false-positive rate divides by nf also when n_rows < nf (utils/metrics.py:151-152).  A split is NaN when nf = 0 or
 *           hi = lo (the reference fails on a flat map: not pinned).  Results are per split; the mean over the splits is the
 *           host's (np.mean), as with p3d_last_eval_shuffled.
 *   AUC-Borji    the sweep with n_rows = nf and idx = randint(0, N, [nf, n_rep]) drawn on the host (utils/metrics.py:139).
 *   Shuffled AUC the sweep with n_rows = min(nf, n_other) and idx the SELECT of the host's ranks in the UNION of M pool slots
 *           (STORE / UNION / SELECT / DRAW ORDER of "Shuffled AUC in the evaluation pass" above, unchanged).
 *   The device never draws.
 * p3d_score_sweep_u8  op level, host arrays: n maps sal / fixation [n][H][W], idx the maps' rows concatenated (nothing for a map
 *                    whose n_rows is 0; may be NULL when every n_rows is 0) -> per_rep [n][n_rep].  Refused before the sweep's
 *                    launch, the outputs untouched: a NULL array, n outside 1 .. 65535, N outside the range, a bad step,
 *                    n_rep < 1, an index outside [0, N), n_rows[b] < 0 or > nf[b] -- nf the device's count (pass A and the
 *                    preparation launch have then run), read back once.
 * p3d_video_shuffled_begin  UNION and its scan for n frames out of the handle's fixation pool (p3d_fixpool_open / p3d_fixpool_put):
 *                    ids [n][M], n_other_out [n] after one synchronisation.  The union is held in buffers of its own: the state
 *                    of p3d_eval_shuffled_begin / _draws, armed or not, is neither read nor disturbed.  Refused as
 *                    p3d_eval_shuffled_begin refuses, and n outside 1 .. 65535; the pool's size is checked at the scoring call.
 *                    p3d_fixpool_open and p3d_fixpool_close drop the held union.
 * p3d_video_score_auc  p3d_video_score's maps chain once, then everything asked for on the same bytes (bit for bit
 *                    p3d_video_maps_u8's under the handle's current settings); pass A runs once per call.  flags != 0: the five
 *                    columns out [n][5] from p3d_video_score's launch descriptions, the same bits; flags = 0 needs out = NULL, and
 *                    density may then be NULL (pass A counts neither hd nor the products).  borji_idx (NULL: no AUC-Borji): every
 *                    frame's [nf][n_rep] indices, concatenated -> borji_per_rep [n][n_rep].  ranks (NULL: no shuffled AUC):
 *                    [n_rows[b]][n_rep] ranks per frame, concatenated -> shuffled_per_rep [n][n_rep]; n_rows[b] must equal
 *                    min(nf[b], n_other[b]) of the held union, the union must be for n frames and the pool for H x W, a rank must
 *                    lie in [0, n_other[b]).  nf is counted from `fixation` on the host and the device's count is held to it.
 *                    Every refusal comes before any launch or upload and leaves the outputs untouched.  stage_ms (or NULL) [4]:
 *                    HIP-event milliseconds of the uploads, of the maps' chain, of the five-column scoring launches (pass A
 *                    included), of the preparation + select + sweeps (0 where no sweep is asked for: nothing is timed).
 * TEST HOOK (tests/test_gpu_score_auc.py):
 * p3d_debug_score_sweep_u8  p3d_score_sweep_u8's launch descriptions with every device buffer between guard elements: sal starts
 *                    `offset` bytes (0 .. 15) past a 16-byte boundary and fixation (3 offset) mod 16 bytes past one, as in
 *                    p3d_debug_score_u8; -1 if a guard or an input changed.  lev_out [n][256], top_out [n][n_rep] (a split's top,
 *                    -1 where nothing is fixated and no row is given) and per_rep come back. */
int p3d_score_sweep_u8(int device, const unsigned char* sal, const unsigned char* fixation, int n, int H, int W, const int* idx,
                       const int* n_rows, int n_rep, double step, double* per_rep);
int p3d_debug_score_sweep_u8(int device, const unsigned char* sal, const unsigned char* fixation, int n, int H, int W, const int* idx,
                             const int* n_rows, int n_rep, double step, int offset, int* lev_out, int* top_out, double* per_rep);
int p3d_video_shuffled_begin(p3d_handle* h, int n, const int* ids, int M, uint32_t* n_other_out);
int p3d_video_score_auc(p3d_handle* h, int first, int n, float scale, int H, int W, const unsigned char* density /* may be NULL */,
                        const unsigned char* fixation, int flags, int ties, double* out /* may be NULL */,
                        const int* borji_idx /* may be NULL */, const int* ranks /* may be NULL */, const int* n_rows, int n_rep,
                        double step, double* borji_per_rep, double* shuffled_per_rep, double* stage_ms /* may be NULL */);

/* ---- Rendering 8-bit maps over their frames (an ADDITION: the arithmetic of what the reference's gen_video.py is for -- a written
 * map laid over the frame it belongs to, colour-mapped, with an iso-line round the salient region; encoding a video container is
 * not part of this library).  OFF until called: every other entry point issues what it issued before and returns the same bits.
 * PARITY UNPINNED: cv2 is not part of the build and the reference has no overlay; this text is the contract and tests/render_ref.py
 * replays it in numpy.  Everything is integer arithmetic, no floating point: no order can show, and every test holds to 0.
 * Per frame: s [H][W] bytes, the saliency map; frame [H][W][3] bytes in cv2's B, G, R order, or absent; table [256], one uint32_t
 * per level v packed b | g << 8 | r << 16 | o << 24, o that level's opacity in 0 .. 255; a contour: level L in 0 .. 255 (0: off),
 * thickness t in 1 .. 4, a colour of three bytes (B, G, R).  -> out [H][W][3] bytes.
 *   BLEND    (b, g, r, o) = table[s], c = (b, g, r); per channel k: out_k = (frame_k * (255 - o) + c_k * o + 127) / 255, integer
 *            division; the largest numerator is 65152.  255 is odd, so no tie exists: this is round-to-nearest of the real blend,
 *            floor(x / 255 + 0.5); o = 255 returns the colour, o = 0 the frame.
 *   Without a frame  out_k = c_k, o is ignored: a plain heat map.
 *   CONTOUR  when L > 0, with a(y, x) = (s(y, x) >= L): a pixel is on the contour exactly when a(y, x) holds and some pixel
 *            (y', x') INSIDE THE MAP with |y' - y| <= t and |x' - x| <= t has a false.  Nothing outside the map counts: a region
 *            that runs into the border gets no line along the border, a map entirely at or above L gets no contour.  A contour
 *            pixel's three bytes are the contour colour; it replaces the blend.
 *   LIMITS   1 <= n <= 65535 maps a call; H, W >= 1; H * W <= 2^28 (3 H W fits int32 inside a map; bases between maps are 64-bit).
 * p3d_render_u8      op level, host arrays: sal [n][H][W], frames [n][H][W][3] or NULL (the heat map), -> out [n][H][W][3].
 * p3d_video_keep_source  legal only while a video is open and before the first p3d_video_put_frames_u8 since the open; anything
 *                    else is refused and changes nothing.  Every p3d_video_open starts with it off.  On: the first
 *                    p3d_video_put_frames_u8 fixes (H0, W0) and allocates a byte store [F][H0][W0][3] (refused, nothing changed,
 *                    if the device cannot hold it); a later put of another size is refused.  The upload lands in the store and
 *                    the normalising launch reads it there, so the stored floats stay, bit for bit, p3d_mapf_frames's.  Frames put
 *                    as floats (p3d_video_put_frames) have no source.  Off: nothing is allocated and the put issues what it issued
 *                    before.
 * p3d_video_source_info  whether the store is on, its frame size (0, 0 until the first put fixes it) and the bytes it holds.
 * p3d_video_render   renders frames first .. first + n - 1 of the open video at H x W.  The saliency bytes are, bit for bit, what
 *                    p3d_video_maps_u8(first, n, scale, H, W) returns under the handle's current settings; maps_out (or NULL)
 *                    receives them.  frames: host [n][H][W][3], uploaded as p3d_video_score uploads its truth, or NULL for the
 *                    kept source -- then H = H0 and W = W0 are required and every frame of the range must have a source (the
 *                    refusal names the first without one).  The heat map without frames exists at op level only.  Validated as
 *                    p3d_video_maps_u8 validates, plus cfg (L in 0 .. 255; with L > 0, t in 1 .. 4) and LIMITS, all before any
 *                    launch, upload or scratch request: a refusal changes nothing.  stage_ms (or NULL) [3]: HIP-event milliseconds
 *                    of the frames' upload (0 with the kept source; the table's 1 KB is not counted), of the maps' chain, of the
 *                    render launch.  Returns synchronised.
 * TEST HOOKS (tests/test_gpu_render.py):
 * p3d_debug_render_u8  the same launch description with every device buffer between guards: sal starts `offset` bytes (0 .. 15)
 *                    past a 16-byte boundary, frames (3 offset) mod 16 and out (5 offset) mod 16 bytes past one, so that offsets 0
 *                    and 8 align the three alike (frame and out bytes of pixel p start at 3 p) and any other offset does not;
 *                    -1 if a guard or an input changed.
 * p3d_debug_render_plan  host only, no HIP call: the block shape of the launch for n maps of H x W with a contour of that thickness
 *                    (0: none).  cols_per_block = 0 (and rows_per_block = 0): the blocks are flat runs of pixels_per_block pixels;
 *                    otherwise tiles of rows_per_block x cols_per_block pixels whose first tile starts at (0, 0). */
typedef struct { uint32_t table[256]; int contour_level, contour_thickness; unsigned char contour_bgr[3]; } p3d_render;
int p3d_render_u8(int device, const unsigned char* sal, const unsigned char* frames /* may be NULL */, int n, int H, int W,
                  const p3d_render* cfg, unsigned char* out);
int p3d_video_keep_source(p3d_handle* h, int on);
int p3d_video_source_info(p3d_handle* h, int* on, int* H0, int* W0, int64_t* bytes);
int p3d_video_render(p3d_handle* h, int first, int n, float scale, int H, int W, const unsigned char* frames /* NULL: kept source */,
                     const p3d_render* cfg, unsigned char* out, unsigned char* maps_out /* may be NULL */, double* stage_ms /* may be NULL */);
int p3d_debug_render_u8(int device, const unsigned char* sal, const unsigned char* frames, int n, int H, int W, const p3d_render* cfg,
                        int offset, unsigned char* out);
int p3d_debug_render_plan(int H, int W, int n, int contour_thickness /* 0: no contour */, int offset,
                          int* rows_per_block, int* cols_per_block, int64_t* pixels_per_block);

/* ---- Reframing around 8-bit maps (an ADDITION: what a video-saliency model is run for -- a smaller window cut out of every frame
 * where the viewers look, on a track steady enough to watch: 16:9 to 9:16, thumbnails, region-of-interest crops for an encoder).
 * OFF until called: every other entry point issues what it issued before and returns the same bits.  PARITY UNPINNED: the reference
 * has nothing of the kind; this text is the contract and tests/reframe_ref.py replays it in numpy.  Everything is integer
 * arithmetic, no floating point anywhere: no order can show, and every test holds to 0.
 * Per frame: s [H][W] bytes, the saliency map; frame [H][W][3] bytes (B, G, R), or absent; a window size hc x wc, 1 <= hc <= H,
 * 1 <= wc <= W; a gate level g in 0 .. 255; a smoothing radius R in 0 .. 255 frames.
 *   LIMITS   1 <= n <= 65535 maps a call; H * W <= 2^23.  The largest mass is 255 * 2^23 < 2^31: one unsigned 32-bit word holds it.
 *   WEIGHT   wt(v) = v where v >= g, else 0; g = 0 weighs every byte by itself.
 *   MASS     for a window with top-left (y0, x0), 0 <= y0 <= H - hc, 0 <= x0 <= W - wc: M(y0, x0) = the sum of wt(s(y, x)) over the
 *            window's hc * wc pixels.  T = the same sum over the whole map.
 *   BEST WINDOW (the raw track)  the window with the largest M; among equals the smallest
 *            D = |2 y0 - (H - hc)| + |2 x0 - (W - wc)| (nearest the centred window); among those the smallest y0, then the smallest
 *            x0.  An all-zero map, a map whose bytes all fall below the gate and a constant map therefore give the centred window,
 *            rounded towards the top-left.
 *   SMOOTHED TRACK  R = 0: the raw track.  Otherwise, over the n frames OF THE CALL, with c(i) = min(max(i, 0), n - 1), separately
 *            per coordinate: Y_f = (2 * sum_{k = -R .. R} y_{c(f + k)} + (2 R + 1)) / (2 (2 R + 1)), integer division, the sum in 64
 *            bits: round-to-nearest, half up, of a box average whose ends repeat the first or last frame.  An average of legal
 *            positions is legal.  The frames of one call are the whole world of the filter: a caller who wants one track for a video
 *            asks for the video in one call.
 *   MASSES   per frame three unsigned 32-bit numbers: M of the best window, M of the window at the smoothed position, T.  Always
 *            M_smoothed <= M_best <= T.
 *   CROP     where frames are present: out[f][y][x][k] = frame[f][Y_f + y][X_f + x][k], out [n][hc][wc][3].  The crop is not
 *            resized: scaling it is the encoder's or the host's job, as video containers are.  Without frames only the tracks and
 *            masses come back.
 * p3d_reframe_u8     op level, host arrays: sal [n][H][W], frames [n][H][W][3] or NULL -> track [n][2] (Y, X), raw [n][2] (or NULL),
 *                    mass [n][3] (or NULL), out [n][hc][wc][3], NULL exactly when frames is.
 * p3d_video_reframe  reframes frames first .. first + n - 1 of the open video at H x W.  The saliency bytes are, bit for bit, what
 *                    p3d_video_maps_u8(first, n, scale, H, W) returns under the handle's current settings; maps_out (or NULL)
 *                    receives them.  out == NULL: tracks and masses only, frames must be NULL too.  Otherwise frames: host
 *                    [n][H][W][3], uploaded as p3d_video_score uploads its truth, or NULL for the source kept by
 *                    p3d_video_keep_source -- then H = H0 and W = W0 are required and every frame of the range must have a source
 *                    (the refusal names the first without one).  Validated as p3d_video_maps_u8 validates, plus cfg, LIMITS, a
 *                    window larger than the map and track == NULL, all before any launch, upload or scratch request: a refusal
 *                    changes nothing.  stage_ms (or NULL) [3] as p3d_video_render's: the frames' upload (0 with the kept source or
 *                    without a crop), the maps' chain, the reframe launches.  Returns synchronised.
 * TEST HOOKS (tests/test_gpu_reframe.py):
 * p3d_debug_reframe_u8  the same launch description with every device buffer, the scratch included, between guards: sal starts
 *                    `offset` bytes (0 .. 15) past a 16-byte boundary, frames (3 offset) mod 16 and out (5 offset) mod 16 bytes past
 *                    one; -1 if a guard or an input changed.
 * p3d_debug_reframe_plan  host only, no HIP call: the window positions a block of the search takes, the search's blocks a map, the
 *                    maps whose summed-area tables are held at a time (a call of more maps runs in chunks of that many) and the bytes
 *                    of scratch the tables and the blocks' bests take. */
typedef struct { int crop_h, crop_w, gate, smooth_radius; } p3d_reframe;
int p3d_reframe_u8(int device, const unsigned char* sal, const unsigned char* frames /* may be NULL */, int n, int H, int W,
                   const p3d_reframe* cfg, int32_t* track /* [n][2]: Y, X */, int32_t* raw /* [n][2], may be NULL */,
                   uint32_t* mass /* [n][3], may be NULL */, unsigned char* out /* [n][crop_h][crop_w][3]; NULL exactly when frames is */);
int p3d_video_reframe(p3d_handle* h, int first, int n, float scale, int H, int W, const unsigned char* frames /* NULL: kept source */,
                      const p3d_reframe* cfg, int32_t* track, int32_t* raw, uint32_t* mass, unsigned char* out /* may be NULL: tracks only */,
                      unsigned char* maps_out /* may be NULL */, double* stage_ms /* may be NULL, [3] as p3d_video_render's */);
int p3d_debug_reframe_u8(int device, const unsigned char* sal, const unsigned char* frames, int n, int H, int W, const p3d_reframe* cfg,
                         int offset, int32_t* track, int32_t* raw, uint32_t* mass, unsigned char* out);
int p3d_debug_reframe_plan(int H, int W, int crop_h, int crop_w, int n, int* positions_per_block, int* search_blocks, int* maps_per_chunk,
                           int64_t* scratch_bytes);

/* ---- Salient regions of 8-bit maps (an ADDITION: what the viewers look at, as objects -- the two faces of a dialogue, a ball and a
 * player, a caption; region-of-interest encoding, multi-subject reframing and annotation all start from this table, and the one
 * window of p3d_video_reframe merges two subjects into the heavier).  OFF until called: every other entry point issues what it issued
 * before and returns the same bits.  PARITY UNPINNED: the reference has nothing of the kind; this text is the contract and
 * tests/regions_ref.py replays it in numpy.  Integer arithmetic throughout: no order can show, and every test holds to 0.
 * Per frame: s [H][W] bytes, the saliency map; a gate g in 1 .. 255; a connectivity c, 4 or 8; a smallest area a >= 1; K in
 * 1 .. P3D_REGIONS_MAX regions kept; link in {0, 1}.
 *   CONFIG      five ints in the order of the P3D_REGIONS_* indices below (an array: `const int cfg[5]`, as the shots configuration
 *               is): gate, connectivity, min_area, max_regions (K), link.
 *   LIMITS      1 <= n <= 65535 maps a call; H * W <= 2^23.  The largest mass is 255 * 2^23 < 2^31, so every field of a region fits
 *               int32_t; the moment sums SY and SX are 64-bit.
 *   FOREGROUND  a pixel is foreground when s(y, x) >= g.  g >= 1: every foreground pixel weighs at least 1 and no region has mass 0.
 *   COMPONENT   a maximal set of foreground pixels connected through 4-neighbours (c = 4) or 8-neighbours (c = 8).  Its ROOT is the
 *               smallest linear index y * W + x among its pixels.
 *   STATISTICS  per component: AREA the pixel count; MASS the sum of the bytes; Y0, X0, Y1, X1 the bounding box, inclusive; PEAK the
 *               largest byte; PEAK_Y, PEAK_X the smallest linear index among the pixels with that byte;
 *               CY = (2 * SY + MASS) / (2 * MASS) with SY = the sum of s(y, x) * y (64-bit, integer division), CX the same with x:
 *               the mass centre rounded to nearest, half up.  It always lies inside the box (not always on a pixel of the region).
 *   SELECTION   only components with AREA >= a are kept; they are ordered by MASS descending, then ROOT ascending; the first K are the
 *               frame's regions, and a region's position in that order is its RANK, 0 .. K - 1.  counts [n][3] holds per frame the
 *               components found, those with AREA >= a, and the regions kept (the smaller of the second count and K).
 *   LABELS      labels [n][H][W] bytes: the rank of the kept region the pixel belongs to, or 255 (background, regions too small,
 *               regions beyond K).
 *   LINK        (link = 1) runs over the frames OF THE CALL.  An optional shot table, in frames of the call (starts [n_shots],
 *               ascending from 0), splits the call into shots; frame 0 of the call and the first frame of every shot are STARTS.  For a
 *               frame f that is not a start: O[j][i] = the number of pixels with labels_f = j and labels_{f-1} = i; PREV(j) = the i
 *               with the largest O[j][i] >= 1, among equals the smallest i, or -1 without any overlap; OVERLAP(j) = O[j][PREV(j)], or
 *               0.  IDs come from one counter that starts at 0 at the call's first frame, never resets and runs in frame order.  At
 *               a start every region takes a new ID, in rank order.  Elsewhere, for every region i of frame f - 1 that is some
 *               PREV(j): its HEIR is, among the j with PREV(j) = i, the one with the largest O[j][i], among equals the smallest j; the
 *               heir takes ID(i).  Every other region of f takes a new ID, in rank order (a region with no overlap, the smaller
 *               part of a split).  A region has one PREV and so inherits at most one ID, and an ID is held by at most one region per
 *               frame; a merged region keeps the ID of the region it overlaps most.  A region that vanishes for a frame comes
 *               back with a new ID.  With link = 0: ID = PREV = -1 and OVERLAP = 0.
 *   RECORD      regions [n][K][P3D_REGION_FIELDS] int32_t, the fields in the order of the P3D_REGION_* indices below.  Slots beyond
 *               the frame's kept count hold -1 in every field.
 * p3d_regions_u8     op level, host arrays: sal [n][H][W], starts [n_shots] or NULL (then n_shots = 0) -> regions, counts (or NULL),
 *                    labels (or NULL).
 * p3d_video_regions  the regions of frames first .. first + n - 1 of the open video at H x W.  The saliency bytes are, bit for bit,
 *                    what p3d_video_maps_u8(first, n, scale, H, W) returns under the handle's current settings; maps_out (or NULL)
 *                    receives them.  The video's shot table, if one is set, is cut to the range exactly as p3d_video_reframe cuts
 *                    it.  Validated as p3d_video_maps_u8 validates, plus cfg, LIMITS and regions == NULL, all before any launch,
 *                    upload or scratch request: a refusal changes nothing.  stage_ms (or NULL) [3]: 0, the maps' chain, the regions
 *                    launches.  Returns synchronised.
 * TEST HOOKS (tests/test_gpu_regions.py):
 * p3d_debug_regions_u8  the same launch description with every device buffer, the scratch included, between guards: sal starts
 *                    `offset` bytes (0 .. 15) past a 16-byte boundary, labels (5 offset) mod 16 bytes past one; -1 if a guard or an
 *                    input changed.
 * p3d_debug_regions_plan  host only, no HIP call: the tile of the labelling (a block a tile), the tiles a map, the maps whose tables
 *                    are held at a time (a call of more maps runs in chunks of that many) and the bytes of scratch, for a call with
 *                    the given K, link and labels (0 or 1: whether the label maps are asked for). */
#define P3D_REGIONS_MAX 64
#define P3D_REGION_FIELDS 15
enum { P3D_REGION_ROOT = 0, P3D_REGION_AREA = 1, P3D_REGION_MASS = 2, P3D_REGION_Y0 = 3, P3D_REGION_X0 = 4, P3D_REGION_Y1 = 5, P3D_REGION_X1 = 6,
       P3D_REGION_PEAK = 7, P3D_REGION_PEAK_Y = 8, P3D_REGION_PEAK_X = 9, P3D_REGION_CY = 10, P3D_REGION_CX = 11, P3D_REGION_ID = 12,
       P3D_REGION_PREV = 13, P3D_REGION_OVERLAP = 14 };
enum { P3D_REGIONS_GATE = 0, P3D_REGIONS_CONNECTIVITY = 1, P3D_REGIONS_MIN_AREA = 2, P3D_REGIONS_MAX_REGIONS = 3, P3D_REGIONS_LINK = 4 };
int p3d_regions_u8(int device, const unsigned char* sal, int n, int H, int W, const int cfg[5], const int32_t* starts /* may be NULL */,
                   int n_shots, int32_t* regions /* [n][max_regions][15] */, int32_t* counts /* [n][3], may be NULL */,
                   unsigned char* labels /* [n][H][W], may be NULL */);
int p3d_video_regions(p3d_handle* h, int first, int n, float scale, int H, int W, const int cfg[5], int32_t* regions,
                      int32_t* counts /* may be NULL */, unsigned char* labels /* may be NULL */, unsigned char* maps_out /* may be NULL */,
                      double* stage_ms /* may be NULL, [3] */);
int p3d_debug_regions_u8(int device, const unsigned char* sal, int n, int H, int W, const int cfg[5], const int32_t* starts, int n_shots,
                         int offset, int32_t* regions, int32_t* counts, unsigned char* labels);
int p3d_debug_regions_plan(int H, int W, int n, int max_regions, int link, int labels, int* tile_h, int* tile_w, int* tiles_per_map,
                           int* maps_per_chunk, int64_t* scratch_bytes);

/* ---- QP maps of 8-bit maps (an ADDITION: what a video encoder takes from a saliency model -- one signed quantiser offset per coding
 * block, 16 x 16 macroblock or 64 x 64 CTU or superblock, lower where the viewers look, steady from frame to frame; the table is about
 * block^2 times smaller than the maps it is made from).  OFF until called: every other entry point issues what it issued before and
 * returns the same bits.  PARITY UNPINNED: the reference has nothing of the kind; this text is the contract and tests/qpmap_ref.py
 * replays it in numpy.  Integer arithmetic throughout: no order can show, and every test holds to 0.  Nothing here drives an encoder
 * or promises one's file format.
 * Per frame: s [H][W] bytes, the saliency map.
 *   CONFIG      nine ints in the order of the P3D_QPMAP_* indices below (an array: `const int cfg[9]`, as the regions configuration
 *               is): block (B), one of 8, 16, 32, 64, 128; peak_weight 0 .. 256; dilate 0 .. 8 blocks; fall and rise 0 .. 254, 0 =
 *               unlimited; balance 0 or 1; target, lo, hi with -127 <= lo <= target <= hi <= 127.  A law `const int32_t law[256]` comes
 *               with it, every entry in -127 .. 127.
 *   LIMITS      1 <= n <= 65535 maps a call; H * W <= 2^23.  Every sum below then fits 32 bits signed: a block sum is at most
 *               255 * 128^2, an area-weighted sum of offsets at most 127 * 2^23.
 *   GRID        Hb = ceil(H / B), Wb = ceil(W / B).  Block (by, bx) covers rows by B .. min(H, (by + 1) B) - 1 and columns likewise;
 *               AREA is its pixel count (edge blocks are partial).
 *   LEVEL       per block: SUM of its bytes and MAX byte; MEAN = (2 SUM + AREA) / (2 AREA), integer division;
 *               L = (peak_weight * MAX + (256 - peak_weight) * MEAN + 128) >> 8, in 0 .. 255.
 *   DILATE      L'(by, bx) = the largest L over the blocks with |dby| <= dilate and |dbx| <= dilate, clipped to the grid (a radius
 *               beyond the grid is legal).
 *   LAW         q0 = law[L'].
 *   LIMIT       runs over the frames OF THE CALL, the whole world of the filter.  An optional shot table, in frames of the call
 *               (starts [n_shots], ascending from 0), splits the call as the regions' LINK is split.  At the call's first frame and at
 *               the first frame of every shot q1 = q0; elsewhere q1_f = min(max(q0_f, q1_{f-1} - fall), q1_{f-1} + rise), a bound
 *               being absent when its field is 0: per block a fast attack and a slow release that never cross a cut.
 *   BALANCE     S1 = the sum over the blocks of AREA * q1, A = H * W.  balance = 1: m = floor((2 S1 + A) / (2 A)), the division
 *               rounding towards minus infinity, and q2 = clamp(q1 + (target - m), lo, hi).  balance = 0: q2 = clamp(q1, lo, hi).
 *               One pass: after the clamp the mean need not equal target, and the statistics say what it is.  The limiter's state
 *               is q1, never q2.
 *   OUTPUTS     qp [n][Hb][Wb] int32_t: q2.  levels [n][Hb][Wb] bytes: L', or NULL.  stats [n][4] int32_t, or NULL: the smallest
 *               q2, the largest q2, S1, and S2 = the sum of AREA * q2.
 * p3d_qpmap_u8       op level, host arrays: sal [n][H][W], law [256], starts [n_shots] or NULL (then n_shots = 0) -> qp, levels (or
 *                    NULL), stats (or NULL).
 * p3d_video_qpmap    the QP maps of frames first .. first + n - 1 of the open video at H x W.  The saliency bytes are, bit for bit,
 *                    what p3d_video_maps_u8(first, n, scale, H, W) returns under the handle's current settings; maps_out (or NULL)
 *                    receives them.  The video's shot table, if one is set, is cut to the range exactly as p3d_video_reframe cuts
 *                    it.  Validated as p3d_video_maps_u8 validates, plus cfg, the law, LIMITS and qp == NULL, all before any launch,
 *                    upload or scratch request: a refusal changes nothing.  stage_ms (or NULL) [3]: 0, the maps' chain, the qpmap
 *                    launches.  Returns synchronised.
 * TEST HOOKS (tests/test_gpu_qpmap.py):
 * p3d_debug_qpmap_u8  the same launch description with every device buffer, the scratch included, between guards: sal starts
 *                    `offset` bytes (0 .. 15) past a 16-byte boundary, levels (5 offset) mod 16 bytes past one; -1 if a guard or an
 *                    input changed.
 * p3d_debug_qpmap_plan  host only, no HIP call: the strip of rows and the tile of columns a block of the reduction takes, the blocks
 *                    a map, the maps whose first levels are held at a time (a call of more maps runs in chunks of that many) and
 *                    the bytes of scratch. */
#define P3D_QPMAP_FIELDS 9
enum { P3D_QPMAP_BLOCK = 0, P3D_QPMAP_PEAK_WEIGHT = 1, P3D_QPMAP_DILATE = 2, P3D_QPMAP_FALL = 3, P3D_QPMAP_RISE = 4, P3D_QPMAP_BALANCE = 5,
       P3D_QPMAP_TARGET = 6, P3D_QPMAP_LO = 7, P3D_QPMAP_HI = 8 };
enum { P3D_QPMAP_STAT_MIN = 0, P3D_QPMAP_STAT_MAX = 1, P3D_QPMAP_STAT_S1 = 2, P3D_QPMAP_STAT_S2 = 3 };
int p3d_qpmap_u8(int device, const unsigned char* sal, int n, int H, int W, const int cfg[9], const int32_t law[256],
                 const int32_t* starts /* may be NULL */, int n_shots, int32_t* qp /* [n][Hb][Wb] */,
                 unsigned char* levels /* [n][Hb][Wb], may be NULL */, int32_t* stats /* [n][4], may be NULL */);
int p3d_video_qpmap(p3d_handle* h, int first, int n, float scale, int H, int W, const int cfg[9], const int32_t law[256], int32_t* qp,
                    unsigned char* levels /* may be NULL */, int32_t* stats /* may be NULL */, unsigned char* maps_out /* may be NULL */,
                    double* stage_ms /* may be NULL, [3] */);
int p3d_debug_qpmap_u8(int device, const unsigned char* sal, int n, int H, int W, const int cfg[9], const int32_t law[256],
                       const int32_t* starts, int n_shots, int offset, int32_t* qp, unsigned char* levels, int32_t* stats);
int p3d_debug_qpmap_plan(int H, int W, int block, int n, int* strip_rows, int* tile_cols, int* blocks_per_map, int* maps_per_chunk,
                         int64_t* scratch_bytes);

/* ---- Pre-filtering frames by their 8-bit maps (an ADDITION: the other way to spend fewer bits where nobody looks, which needs no
 * cooperation from an encoder -- the frame is low-pass filtered where the viewers do not look and left bit-exact where they do, the
 * strength changing smoothly in space and slowly in time; any encoder takes the result).  OFF until called: every other entry point
 * issues what it issued before and returns the same bits.  PARITY UNPINNED: the reference has nothing of the kind; this text is the
 * contract and tests/prefilter_ref.py replays it in numpy.  Integer arithmetic throughout, no floating point: no order can show, and
 * every test holds to 0.  Nothing here drives an encoder or says what bitrate one saves.
 * Per frame: s [H][W] bytes, the saliency map; frame [H][W][3] bytes in cv2's B, G, R order.  -> out [H][W][3] bytes.
 *   CONFIG      seven ints in the order of the P3D_PREFILTER_* indices below (an array, `const int cfg[P3D_PREFILTER_FIELDS]`, as the
 *               QP maps' configuration is): block (B), one of 8, 16, 32, 64, 128; peak_weight 0 .. 256; dilate 0 .. 8 blocks; fall and
 *               rise 0 .. 64, 0 = unlimited; radius (R) 1 .. 16; passes (P) 1 .. 3.  A law `const int32_t law[256]` comes with it,
 *               every entry in 0 .. 64: 64 is the full low-pass, 0 leaves the frame alone, and a law meant for use falls with the
 *               level.
 *   LIMITS      1 <= n <= 65535 maps a call; H * W <= 2^23.  Frames are required: there is no frame-less form.
 *   STRENGTH GRID  g [n][Hb][Wb] is, by definition, the qp that "QP maps of 8-bit maps" above gives for the same maps with block = B,
 *               the same peak_weight, dilate, fall and rise, balance = 0, target = 0, lo = 0, hi = 64, this law and this shot table:
 *               GRID, LEVEL, DILATE, LAW and LIMIT of that section, word for word.  So 0 <= g <= 64; rise bounds how fast the
 *               smoothing comes on from frame to frame, fall how fast it goes away, and neither crosses the start of a shot.
 *   PIXEL WEIGHT  interpolates g between block centres; an edge block's centre is taken as if the block were whole.  D = 2 B.  For
 *               row y: u = 2 y + 1 - B, j0 = floor(u / D) (towards minus infinity), fy = u - D j0 in 0 .. D - 1,
 *               ja = clamp(j0, 0, Hb - 1), jb = clamp(j0 + 1, 0, Hb - 1); for column x: i0, fx, ia, ib likewise from W and Wb.
 *               Wn(y, x) = (D - fy)(D - fx) g[ja][ia] + (D - fy) fx g[ja][ib] + fy (D - fx) g[jb][ia] + fy fx g[jb][ib], in 0 .. Q,
 *               Q = 64 D^2 = 2^(8 + 2 log2 B).
 *   LOW-PASS    per channel k: l_0 = frame; for p = 1 .. P, SUM = the sum of l_{p-1}(clamp(y + dy, 0, H - 1), clamp(x + dx, 0, W - 1), k)
 *               over |dy| <= R and |dx| <= R, A = (2 R + 1)^2, l_p(y, x, k) = (2 SUM + A) / (2 A), integer division; low = l_P.
 *               Borders replicate, so A is one constant and a radius beyond the frame is legal; SUM <= 255 * 1089.  Each pass
 *               rounds once, on the 2-D sum: the sum is separable, the rounding is not.
 *   BLEND       out_k = (frame_k (Q - Wn) + low_k Wn + Q / 2) >> log2 Q; the largest numerator is below 2^31.  Wn = 0 returns the
 *               frame's bytes, Wn = Q returns low, and a constant frame returns itself under any setting.
 *   OUTPUTS     out [n][H][W][3] bytes.  grid [n][Hb][Wb] int32_t: g, or NULL.
 * p3d_prefilter_u8   op level, host arrays: sal [n][H][W], frames [n][H][W][3], law [256], starts [n_shots] or NULL (then n_shots = 0)
 *                    -> out, grid (or NULL).
 * p3d_video_prefilter  filters frames first .. first + n - 1 of the open video at H x W.  The saliency bytes are, bit for bit, what
 *                    p3d_video_maps_u8(first, n, scale, H, W) returns under the handle's current settings; maps_out (or NULL)
 *                    receives them.  frames: host [n][H][W][3], uploaded as p3d_video_render uploads its frames, or NULL for the
 *                    kept source -- then H = H0 and W = W0 are required and every frame of the range must have a source.  The
 *                    video's shot table, if one is set, is cut to the range exactly as p3d_video_qpmap cuts it.  Validated as
 *                    p3d_video_maps_u8 validates, plus cfg, the law, LIMITS and out == NULL, all before any launch, upload or scratch
 *                    request: a refusal changes nothing.  stage_ms (or NULL) [3]: the frames' upload (0 with the kept source), the
 *                    maps' chain, the prefilter launches (the grid's and the filter's).  Returns synchronised.
 * TEST HOOKS (tests/test_gpu_prefilter.py):
 * p3d_debug_prefilter_u8  the same launch description with every device buffer, the scratch included, between guards: sal starts
 *                    `offset` bytes (0 .. 15) past a 16-byte boundary, frames (3 offset) mod 16 and out (5 offset) mod 16 bytes past
 *                    one; -1 if a guard or an input changed.
 * p3d_debug_prefilter_plan  host only, no HIP call, for n frames of H x W with block B, radius R and P passes: the tile of output
 *                    rows and columns a block takes (the first tile starts at (0, 0)); the halo in pixels a block reads round its
 *                    tile; fused = 1 when the P passes run inside one launch (halo = R P), 0 when each is a launch through memory
 *                    (halo = R); the blocks a frame; the frames whose intermediate passes are held at a time (a call of more frames
 *                    runs in chunks of that many); the bytes of scratch of those intermediate passes; and mul and shift with
 *                    floor(x / (2 (2 R + 1)^2)) = (x * mul) >> shift for every 0 <= x <= 2 * 255 * (2 R + 1)^2 + (2 R + 1)^2, the
 *                    product taken in 64 bits: how the kernel divides. */
#define P3D_PREFILTER_FIELDS 7
enum { P3D_PREFILTER_BLOCK = 0, P3D_PREFILTER_PEAK_WEIGHT = 1, P3D_PREFILTER_DILATE = 2, P3D_PREFILTER_FALL = 3, P3D_PREFILTER_RISE = 4,
       P3D_PREFILTER_RADIUS = 5, P3D_PREFILTER_PASSES = 6 };
int p3d_prefilter_u8(int device, const unsigned char* sal, const unsigned char* frames, int n, int H, int W, const int cfg[7],
                     const int32_t law[256], const int32_t* starts /* may be NULL */, int n_shots, unsigned char* out /* [n][H][W][3] */,
                     int32_t* grid /* [n][Hb][Wb], may be NULL */);
int p3d_video_prefilter(p3d_handle* h, int first, int n, float scale, int H, int W, const unsigned char* frames /* NULL: kept source */,
                        const int cfg[7], const int32_t law[256], unsigned char* out, int32_t* grid /* may be NULL */,
                        unsigned char* maps_out /* may be NULL */, double* stage_ms /* may be NULL, [3] */);
int p3d_debug_prefilter_u8(int device, const unsigned char* sal, const unsigned char* frames, int n, int H, int W, const int cfg[7],
                           const int32_t law[256], const int32_t* starts, int n_shots, int offset, unsigned char* out, int32_t* grid);
int p3d_debug_prefilter_plan(int H, int W, int block, int radius, int passes, int n, int* tile_rows, int* tile_cols, int* halo, int* fused,
                             int* blocks_per_frame, int* frames_per_chunk, int64_t* scratch_bytes, uint32_t* mul, int* shift);

/* ---- Distortion of frames under their 8-bit maps (an ADDITION: what a change to the frames -- a pre-filter, an encoder driven by the
 * QP maps -- cost where the viewers look and what it cost elsewhere; the literature reports it as saliency-weighted PSNR, and SSIM
 * is expected beside it).  OFF until called: every other entry point issues what it issued before and returns the same bits.
 * PARITY UNPINNED: the reference has nothing of the kind; this text is the contract and tests/distortion_ref.py replays it in numpy.
 * The device leaves integers only, and every integer test holds to 0; PSNR and SSIM are then a few float64 operations on the host
 * (dataflow.distortion_report).  Nothing here drives an encoder or says what bitrate one saves.
 * Per frame: s [H][W] bytes, the saliency map; ref [H][W][3] and test [H][W][3] bytes in cv2's B, G, R order.
 *   CONFIG      two ints in the order of the P3D_DISTORTION_* indices below (an array, `const int cfg[P3D_DISTORTION_FIELDS]`):
 *               block, 0 (no block map) or one of 8, 16, 32, 64, 128; gate 0 .. 255, 0 = off.  A weight law
 *               `const int32_t wlaw[256]` comes with it, every entry in 0 .. 255: per pixel w = wlaw[s].
 *   LIMITS      1 <= n <= 65535 frames a call; H * W <= 2^23.  test is required; so is ref, except where an entry point names what
 *               stands in for it.
 *   PLANES      four, k = 0 .. 3: B, G, R and Y = (29 B + 150 G + 77 R + 128) >> 8 (the coefficients sum to 256: Y is in 0 .. 255).
 *               d_k = ref_k - test_k; Y's difference is the difference of the two frames' Y values.
 *   RECORD      int64_t table [n][P3D_DISTORTION_RECORD], the sums over the frame's pixels under the P3D_DISTORTION_* indices:
 *               SSE + k: sum of d_k^2 (<= 65025 * 2^23 < 2^39).  WSSE + k: sum of w d_k^2 (<= 255 * 65025 * 2^23 < 2^47, the largest
 *               sum here).  SW: sum of w (< 2^31).  MAXABS + k: the largest |d_k| (<= 255).  CHANGED: the pixels where any of the
 *               three B, G, R bytes differ.  SALIENT: the pixels with s >= gate, 0 when gate = 0.  CHANGED_SALIENT: the pixels
 *               that are both (all three <= 2^23).  NW, SQ, SWQ, SWW: SSIM below.
 *   SSIM        on Y alone, made of integers.  Windows are 8 x 8 pixels at stride 4 on both axes: a window's top-left corner is
 *               row 4 j, column 4 i for every j, i >= 0 with 4 j + 8 <= H and 4 i + 8 <= W.  NW is their count (<= 2^19); H < 8 or
 *               W < 8 gives NW = SQ = SWQ = SWW = 0.  Per window five sums over its 64 pixels, a = ref's Y and b = test's Y:
 *               sa, sb, saa, sbb, sab.  c1 = 26634 = round(4096 * 6.5025), c2 = 235963 = round(64 * 63 * 58.5225) (the variance
 *               is the unbiased one).  num = (2 sa sb + c1) (2 (64 sab - sa sb) + c2),
 *               den = (sa^2 + sb^2 + c1) (64 (saa + sbb) - sa^2 - sb^2 + c2): int64, below 2^56 in magnitude, den > 0, num may be
 *               negative.  q = floor(double(num) / double(den) * 65536 + 0.5) as an integer, in -65536 .. 65536: one correctly
 *               rounded conversion of an int64 to a double each, one IEEE division; the multiplication by 2^16 is exact, so its
 *               contraction with the addition into a fused multiply-add gives the same value.  (distortion.hip is built
 *               without fast-math, as every file of the library is: a reciprocal in place of the division would break this.)
 *               ww = the sum of w over the window's 64 pixels.  SQ = sum of q; SWQ = sum of ww q (< 2^49); SWW = sum of ww
 *               (< 2^33).  q is quantised before it is summed, so no order of summation can show: SSIM holds to 0 like the rest.
 *   BLOCK MAP   int64_t block_sse [n][Hb][Wb], or NULL: the sum of d_B^2 + d_G^2 + d_R^2 over the block (<= 3 * 65025 * 2^14);
 *               Hb, Wb and the edge blocks as GRID of "QP maps of 8-bit maps".  Required to be NULL when block = 0, and optional
 *               otherwise.
 * p3d_distortion_u8   op level, host arrays: sal [n][H][W], ref and test [n][H][W][3], wlaw [256] -> table, block_sse (or NULL).
 * p3d_video_distortion  compares frames first .. first + n - 1 of the open video at H x W.  The saliency bytes are, bit for bit,
 *                    what p3d_video_maps_u8(first, n, scale, H, W) returns under the handle's current settings; maps_out (or
 *                    NULL) receives them.  test: host [n][H][W][3], uploaded as p3d_video_render uploads its frames.  ref:
 *                    likewise, or NULL for the kept source -- then H = H0 and W = W0 are required and every frame of the range
 *                    must have a source.  Validated as p3d_video_maps_u8 validates, plus cfg, the law, LIMITS, test == NULL,
 *                    table == NULL and a block map with block = 0, all before any launch, upload or scratch request: a refusal
 *                    changes nothing.  stage_ms (or NULL) [3]: the frames' upload, the maps' chain, the distortion launches.
 *                    Returns synchronised.
 * TEST HOOKS (tests/test_gpu_distortion.py):
 * p3d_debug_distortion_u8  the same launch description with every device buffer between guards: sal starts `offset` bytes (0 .. 15)
 *                    past a 16-byte boundary, ref (3 offset) mod 16 and test (5 offset) mod 16 bytes past one; -1 if a guard or an
 *                    input changed.
 * p3d_debug_distortion_plan  host only, no HIP call, for n frames of H x W with this block (0: no block map): the tile of rows and
 *                    columns a block of the sums' launch takes (the first tile starts at (0, 0)); the blocks a frame of that
 *                    launch; the rows and columns of SSIM windows a frame (their product is NW); the bytes of scratch beyond the
 *                    outputs (0: the sums meet in the table through 64-bit integer atomics, whose order cannot show). */
#define P3D_DISTORTION_FIELDS 2
enum { P3D_DISTORTION_BLOCK = 0, P3D_DISTORTION_GATE = 1 };
#define P3D_DISTORTION_RECORD 20
enum { P3D_DISTORTION_SSE = 0, P3D_DISTORTION_WSSE = 4, P3D_DISTORTION_SW = 8, P3D_DISTORTION_MAXABS = 9, P3D_DISTORTION_CHANGED = 13,
       P3D_DISTORTION_SALIENT = 14, P3D_DISTORTION_CHANGED_SALIENT = 15, P3D_DISTORTION_NW = 16, P3D_DISTORTION_SQ = 17,
       P3D_DISTORTION_SWQ = 18, P3D_DISTORTION_SWW = 19 };
int p3d_distortion_u8(int device, const unsigned char* sal, const unsigned char* ref, const unsigned char* test, int n, int H, int W,
                      const int cfg[2], const int32_t wlaw[256], int64_t* table /* [n][P3D_DISTORTION_RECORD] */,
                      int64_t* block_sse /* [n][Hb][Wb], may be NULL */);
int p3d_video_distortion(p3d_handle* h, int first, int n, float scale, int H, int W, const unsigned char* ref /* NULL: kept source */,
                         const unsigned char* test, const int cfg[2], const int32_t wlaw[256], int64_t* table,
                         int64_t* block_sse /* may be NULL */, unsigned char* maps_out /* may be NULL */,
                         double* stage_ms /* may be NULL, [3] */);
int p3d_debug_distortion_u8(int device, const unsigned char* sal, const unsigned char* ref, const unsigned char* test, int n, int H, int W,
                            const int cfg[2], const int32_t wlaw[256], int offset, int64_t* table, int64_t* block_sse);
int p3d_debug_distortion_plan(int H, int W, int block, int n, int* tile_rows, int* tile_cols, int* blocks_per_frame, int* window_rows,
                              int* window_cols, int64_t* scratch_bytes);

/* ---- Shot boundaries of 8-bit frames (an ADDITION: the videos people reframe are edited, and a filter along the frame axis that
 * runs across a hard cut blends two unrelated scenes; automatic reframing tools find the cuts first).  OFF until called: every other
 * entry point issues what it issued before and returns the same bits.  PARITY UNPINNED: the reference's clips are single takes and
 * it has nothing of the kind; this text is the contract and tests/shots_ref.py replays it in numpy.  SIGNAL and DECISION are integer
 * arithmetic, no floating point anywhere: no order can show, and every test holds to 0.  Hard cuts only: a dissolve or a fade
 * spreads its change over many frames, none of which is a peak, and is NOT detected by the entry points of this section; "Gradual
 * transitions" below finds them, behind entry points of its own.
 * Per frame: bytes [H][W][3] (B, G, R); a grid of gy x gx cells, 1 <= gy <= min(P3D_SHOTS_MAX_GRID, H), 1 <= gx <= min(.., W).
 *   LIMITS   1 <= n <= 65535 frames a call; P = H * W <= 2^28, so that 6 P fits 32 bits.
 *   CELL     pixel (y, x) lies in cell (y * gy / H, x * gx / W), integer division.
 *   HIST     per cell and channel 64 bins, bin = byte >> 2; counts are unsigned 32-bit.
 *   DIST     D_0 = 0; for f >= 1, D_f = the sum over cells, channels and bins of |h_f - h_{f-1}|.  0 <= D_f <= 6 P.
 *   CONFIG   six ints in the order of the P3D_SHOTS_* indices below (an array: `const int cfg[6]`): grid_y, grid_x; threshold_permille
 *            in 1 .. 1000; window in 0 .. 32; ratio_q8 in 256 .. 65535; min_length >= 1.
 *   CAND(f)  for 1 <= f <= F - 1, in 64-bit integers: D_f * 1000 >= threshold_permille * 6 * P, and D_f * 256 >= ratio_q8 * N_f,
 *            where N_f is the largest D_g over g != f, 1 <= g <= F - 1, |g - f| <= window (0 where there is no such g, so also for
 *            window = 0).  The second test is the peak rule: a flash -- one bright frame, two large distances side by side -- fails
 *            it at any ratio above 256 times the smaller over the larger.
 *   ACCEPT   f ascending, last = 0: f starts a shot exactly when CAND(f), f - last >= min_length and F - f >= min_length; then
 *            last = f.
 *   RESULT   starts [n_shots], strictly ascending, starts[0] = 0: shot k is frames starts[k] .. starts[k + 1] - 1, the last to F - 1.
 * p3d_shot_distances_u8  op level, host frames [n][H][W][3] -> D [n].
 * p3d_shot_cuts          op level, host D [F] and P = H * W of its frames -> the first min(cap, n_shots) starts and n_shots (cap >= 1).
 *                        The decision runs on the device, one block behind the signal's launches; grid_y and grid_x are not read.
 * Refused (-1, p3d_last_error set, nothing launched): a null pointer, LIMITS, a grid or a CONFIG value outside its range.
 * TEST HOOKS (tests/test_gpu_shots.py):
 * p3d_debug_shot_distances_u8  the same launch description with every device buffer, the scratch included, between guards; the frames
 *                        start `offset` bytes (0 .. 15) past a 16-byte boundary; ballot 1 counts a wave's equal bins with one add
 *                        (score_u8.hip's way), 0 adds every byte on its own: the same D.  -1 if a guard or the frames changed.
 * p3d_debug_shots_plan   host only, no HIP call: the rows a block of the count takes, its blocks a frame, the frames whose tables are
 *                        held at a time (a call of more frames runs in chunks of that many, each seeded with the last table of the
 *                        one before) and the bytes of scratch the tables take.
 * p3d_debug_shots_time   HIP-event milliseconds of `reps` rounds of: the signal's launches without and with ballot, and a
 *                        device-to-device copy of the same n * H * W * 3 bytes (the roof of a kernel that reads every byte once), in
 *                        turn, after one untimed round.
 * THE OPEN VIDEO'S SHOT TABLE.  p3d_video_open starts without one and nothing reads one until it is installed; a refusal changes
 * nothing and launches nothing.
 * p3d_video_set_shots     installs starts [n_shots]: starts[0] == 0, strictly ascending, every start < F; NULL removes the table.
 * p3d_video_get_shots     the first min(cap, n_shots) starts (starts may be NULL) and n_shots, 0 without a table.
 * p3d_video_detect_shots  SIGNAL and DECISION on the source kept by p3d_video_keep_source, F <= 65535 frames at H0 x W0: refused
 *                         unless every frame has a source (the error names the first without one).  D_out [F] and starts_out [cap]
 *                         may be NULL; n_shots receives the number of shots; install != 0 installs the table.
 * p3d_video_shots_last_ms HIP-event ms [2] of the last detection: the signal's launches, the decision.
 * While a table is installed, frame f lying in shot [lo, hi], L = hi - lo + 1:
 *   TEMPORAL  (the stage of p3d_set_video_temporal, while on; float32, each operation rounding on its own: bit for bit)
 *     GAUSS   the PASS of that section with rho replaced by rho_s(i) = lo + refl(i - lo, L); refl(j, 1) = 0, otherwise with
 *             m = j mod (2 L - 2), non-negative, refl = m where m < L, else 2 L - 2 - m: periodic reflect-101, so a shot of any
 *             length is legal and the read-out refusal r > F - 1 does not apply.  A read needs, of every shot it touches in frames
 *             a .. b, frames max(lo, a - r) .. min(hi, b + r).  One shot and r <= F - 1: the bits without a table.
 *     EMA     m_lo = v_lo, a copy of the bits: the recurrence restarts at every shot.  A read needs frames lo(first) .. first + n - 1,
 *             and the bits of a partial read are the slice of a full read.
 *   REFRAME   p3d_video_reframe's SMOOTHED TRACK takes c(i) = min(max(i, a), b), [a, b] the frame's shot intersected with the frames
 *             of the call: the ends of a shot repeat and the window may jump at a cut.  BEST WINDOW, MASSES and CROP are unchanged.
 *   p3d_video_predict's windows straddle cuts by design, table or no table; p3d_video_predict_shots ("Shot-aware windows" below)
 *   keeps every window inside its shot.  p3d_video_score and p3d_video_render do not read the table.
 * p3d_temporal_filter_shots  the temporal stage alone under a table, on a host store [F][hw] and counts [F] (NULL: every count 1)
 *                         under `mode`, frames first .. first + n - 1 -> out [n][hw]; every device buffer, the run table included,
 *                         sits between guards, the floats `offset` (0 .. 3) elements past a 16-byte boundary.
 * p3d_reframe_shots_u8    p3d_reframe_u8 under a table starts [n_shots] over the n frames of the call; offset -1: the stage on the
 *                         stream's scratch, as p3d_reframe_u8; 0 .. 15: between guards and shifted, as p3d_debug_reframe_u8. */
#define P3D_SHOTS_MAX_GRID 4
enum { P3D_SHOTS_GRID_Y = 0, P3D_SHOTS_GRID_X = 1, P3D_SHOTS_THRESHOLD = 2, P3D_SHOTS_WINDOW = 3, P3D_SHOTS_RATIO = 4, P3D_SHOTS_MIN_LENGTH = 5 };
int p3d_shot_distances_u8(int device, const unsigned char* frames, int n, int H, int W, int grid_y, int grid_x, uint32_t* D /* [n] */);
int p3d_shot_cuts(int device, const uint32_t* D, int F, int64_t P, const int cfg[6], int32_t* starts /* [cap] */, int cap, int* n_shots);
int p3d_debug_shot_distances_u8(int device, const unsigned char* frames, int n, int H, int W, int grid_y, int grid_x, int offset, int ballot,
                                uint32_t* D);
int p3d_debug_shots_plan(int H, int W, int grid_y, int grid_x, int n, int* rows_per_block, int* blocks_per_frame, int* frames_per_chunk,
                         int64_t* scratch_bytes);
int p3d_debug_shots_time(int device, const unsigned char* frames, int n, int H, int W, int grid_y, int grid_x, int reps,
                         double* signal_ms /* [reps] */, double* ballot_ms /* [reps] */, double* copy_ms /* [reps] */);
int p3d_video_set_shots(p3d_handle* h, const int32_t* starts /* NULL: remove */, int n_shots);
int p3d_video_get_shots(p3d_handle* h, int32_t* starts /* [cap], may be NULL */, int cap, int* n_shots);
int p3d_video_detect_shots(p3d_handle* h, const int cfg[6], uint32_t* D_out /* [F], may be NULL */, int32_t* starts_out /* [cap], may be NULL */,
                           int cap, int* n_shots, int install);
int p3d_video_shots_last_ms(p3d_handle* h, double* ms /* [2] */);
int p3d_temporal_filter_shots(int device, int mode, const p3d_video_temporal* cfg, const float* store, const int32_t* count /* may be NULL */,
                              int F, int64_t hw, const int32_t* starts, int n_shots, int first, int n, int offset, float* out);
int p3d_reframe_shots_u8(int device, const unsigned char* sal, const unsigned char* frames /* may be NULL */, int n, int H, int W,
                         const p3d_reframe* cfg, const int32_t* starts, int n_shots, int offset /* -1, or 0 .. 15 */, int32_t* track,
                         int32_t* raw /* may be NULL */, uint32_t* mass /* may be NULL */, unsigned char* out /* NULL exactly when frames is */);

/* ---- Gradual transitions (an ADDITION beside the hard-cut detector above: edited video is full of dissolves and fades to black,
 * and across one the temporal filter, the reframe track and the network's windows still mix two scenes).  OFF until called: every
 * entry point above issues what it issued before and returns the same bits.  PARITY UNPINNED, as above: this text is the contract and
 * tests/transitions_ref.py replays it in numpy and Python integers; every test holds to 0.  Frames, grid, LIMITS, CELL, HIST, DIST,
 * CAND and the cut CONFIG cfg[6] are those of "Shot boundaries of 8-bit frames"; P = H * W.
 *   SIGNAL   three numbers a frame, all from the cell histograms h_f:
 *            D_f  exactly DIST.
 *            E_f  for a lag K in 2 .. 64: 0 for f < K, otherwise the sum over cells, channels and bins of |h_f - h_{f-K}|.
 *                 0 <= E_f <= 6 P.  K = 0: E_f = 0 for every f.
 *            v_f  the spread, independent of the grid: per channel c, n_b = the sum of bin b over all cells, S1 = sum b n_b and
 *                 S2 = sum b^2 n_b over b = 0 .. 63, w_c = S2 - floor(S1^2 / P); v_f = w_0 + w_1 + w_2, 0 <= v_f < 2^40, int64.
 *                 S1^2 reaches 2^68 and is not formed: with q = S1 / P and r = S1 - q P, floor(S1^2 / P) = q^2 P + 2 q r +
 *                 floor(r^2 / P), every term below 2^64.
 *   CONFIG   five ints beside cfg[6], in the order of the P3D_GRADUAL_* indices below (`const int gcfg[5]`): LAG, the lag K, 0
 *            (dissolves off) or 2 .. 64; HIGH, permille, 1 .. 1000; DIP, q8, 1 .. 256; MONO, q8, 0 .. 65535; MONO_MIN, frames, 0
 *            (fades off) or >= 1.  The drivers' defaults: 12, 250, 230, 768, 2.
 *   DECISION in 64-bit integers:
 *     MONO(f)  v_f * 256 <= MONO * P.
 *     FADE     every maximal run [a, b] of MONO frames with b - a + 1 >= MONO_MIN, a >= 1 and b <= F - 2 sets FADE(b + 1): the next
 *              shot starts at the first frame that is no longer monochrome, the fade-out and the black frames stay with the shot
 *              before.  MONO_MIN = 0: no FADE.
 *     HIGH(f)  K >= 2, f >= K and E_f * 1000 >= HIGH * 6 * P.
 *     DISS     every maximal run [p, q] of HIGH frames, n = q - p + 1, sets DISS(s), s = (p + q - K + 1) >> 1, when all four hold:
 *              LENGTH   2 n >= K and n <= 2 K;
 *              NO CUT   no g in [max(1, p - K + 1), q] has CAND(g) (a hard cut makes a bump of K frames in E by itself);
 *              NO MONO  no g in [max(0, p - K), q] has MONO(g) (fades belong to FADE);
 *              DIP      with lo = max(p - K, 0): 256 * the least v over [lo, q] <= DIP * min(v_lo, v_q) -- the variance dip of a
 *                       blend of two uncorrelated scenes, which a pan or a brightness drift does not have.  DIP = 256: always true.
 *              A hard cut at a would give s = a; a linear dissolve over frames a .. a + L - 1 gives s about a + L / 2.
 *     KIND(f)  P3D_SHOT_CUT if CAND(f), else P3D_SHOT_FADE if FADE(f), else P3D_SHOT_DISSOLVE if DISS(f), else none.
 *     ACCEPT   the ACCEPT above with "KIND(f) is not none" in place of CAND(f).
 *   RESULT   starts [n_shots] as above and kinds [n_shots], kinds[0] = P3D_SHOT_FIRST, kinds[k] = KIND(starts[k]).  With LAG = 0 and
 *            MONO_MIN = 0 the starts are p3d_shot_cuts's for every input.
 *   NOT FOUND: a dissolve longer than about K frames (LENGTH fails); a wipe.  A pan that starts and stops within about K frames is
 *            rejected by DIP alone.
 * p3d_shot_signals_u8   op level, host frames [n][H][W][3] -> D, E [n] and v [n]; lag is K, 0 or 2 .. 64.
 * p3d_shot_transitions  op level, host D, E, v [F] (every v in [0, 2^40)) and P -> the first min(cap, n_shots) starts and kinds, and
 *                       n_shots (cap >= 1).  One block on the device; every buffer between guards; grid_y and grid_x are not read.
 * p3d_video_detect_transitions  SIGNAL and DECISION on the kept source, as p3d_video_detect_shots and with its refusals; D_out, E_out,
 *                       v_out [F], starts_out and kinds_out [cap] may be NULL; install != 0 installs the table and its kinds.
 * p3d_video_get_shot_kinds  the first min(cap, n_shots) kinds of the installed table (kinds may be NULL) and n_shots, 0 without a
 *                       table.  A table of p3d_video_set_shots or p3d_video_detect_shots has P3D_SHOT_CUT for every shot after the first.
 * p3d_video_shots_last_ms reports the last detection of either kind.
 * Refused (-1, p3d_last_error set, nothing launched): a null pointer, LIMITS, a grid or a value of either CONFIG outside its range.
 * TEST HOOKS (tests/test_gpu_transitions.py, tests/test_transitions_cpu.py):
 * p3d_debug_shot_signals_u8   the signal's launch description with every device buffer, the scratch included, between guards; the
 *                       frames start `offset` bytes (0 .. 15) past a 16-byte boundary.  -1 if a guard or the frames changed.
 * p3d_debug_transitions_plan  host only, no HIP call: tables = min(n, 64) + max(K, 1) tables of grid_y * grid_x * 192 words are held
 *                       (a chunk of at most 64 frames behind the last max(K, 1) tables of the chunk before), scratch_bytes = 4 bytes
 *                       a word.
 * p3d_debug_transitions_time  HIP-event milliseconds of `reps` rounds of: the cut signal's launches (p3d_shot_distances_u8's) and
 *                       this section's signal launches on the same frames, in turn, after one untimed round. */
enum { P3D_GRADUAL_LAG = 0, P3D_GRADUAL_HIGH = 1, P3D_GRADUAL_DIP = 2, P3D_GRADUAL_MONO = 3, P3D_GRADUAL_MONO_MIN = 4 };
enum { P3D_SHOT_FIRST = 0, P3D_SHOT_CUT = 1, P3D_SHOT_FADE = 2, P3D_SHOT_DISSOLVE = 3 };
int p3d_shot_signals_u8(int device, const unsigned char* frames, int n, int H, int W, int grid_y, int grid_x, int lag, uint32_t* D /* [n] */,
                        uint32_t* E /* [n] */, int64_t* v /* [n] */);
int p3d_shot_transitions(int device, const uint32_t* D, const uint32_t* E, const int64_t* v, int F, int64_t P, const int cfg[6],
                         const int gcfg[5], int32_t* starts /* [cap] */, int32_t* kinds /* [cap] */, int cap, int* n_shots);
int p3d_video_detect_transitions(p3d_handle* h, const int cfg[6], const int gcfg[5], uint32_t* D_out /* [F], may be NULL */,
                                 uint32_t* E_out /* [F], may be NULL */, int64_t* v_out /* [F], may be NULL */,
                                 int32_t* starts_out /* [cap], may be NULL */, int32_t* kinds_out /* [cap], may be NULL */, int cap,
                                 int* n_shots, int install);
int p3d_video_get_shot_kinds(p3d_handle* h, int32_t* kinds /* [cap], may be NULL */, int cap, int* n_shots);
int p3d_debug_shot_signals_u8(int device, const unsigned char* frames, int n, int H, int W, int grid_y, int grid_x, int lag, int offset,
                              uint32_t* D, uint32_t* E, int64_t* v);
int p3d_debug_transitions_plan(int H, int W, int grid_y, int grid_x, int n, int lag, int* tables, int64_t* scratch_bytes);
int p3d_debug_transitions_time(int device, const unsigned char* frames, int n, int H, int W, int grid_y, int grid_x, int lag, int reps,
                               double* cut_ms /* [reps] */, double* signal_ms /* [reps] */);

/* ---- Shot-aware windows (an ADDITION beside p3d_video_predict, whose windows are T consecutive frames wherever the cuts lie: a
 * window across a cut shows the network a clip of two unrelated scenes, and every map within T - 1 frames of the cut is predicted
 * from it).  p3d_video_predict_shots keeps every window inside the shot of its start in the installed table; p3d_video_predict
 * itself is unchanged, with or without a table, and nothing is allocated until the first call (the per-call slot table [B * T],
 * freed with the video).  PARITY UNPINNED: the reference has no shots, so this text is the contract and tests/shot_windows_ref.py
 * replays it in numpy bit for bit.  T, B, F as in "Resident video inference".  Needs an open video with a shot table.
 * For window k, s = starts[k], [lo, hi] the shot of s in the installed table and L = hi - lo + 1:
 *   LEGAL    n_windows in 1 .. B; starts strictly ascending, every start greater than last_start and inside [0, F - 1]; and
 *            s == lo, or s + T - 1 <= hi.  So a shot of at least T frames takes any window that lies wholly inside it, and a shorter
 *            shot takes exactly one window, at its first frame.
 *   SLOTS    slot t of clip k reads frame g(k, t) = lo + refl(s - lo + t, L), refl the periodic reflect-101 of TEMPORAL above
 *            (refl(j, 1) = 0, otherwise m = j mod (2 L - 2), and m where m < L, else 2 L - 2 - m).  For a window inside its shot this
 *            is the identity; no slot ever leaves [lo, hi].  Every frame g(k, t) must have been put.
 *   LIVE     live(k) = min(T, hi - s + 1).  Slots t < live(k) are frame s + t itself and are the only ones folded into the map store;
 *            the reflected slots are padding for the network: their predictions are dropped and the scatter does not read them.
 *   GATHER   one launch: clip k, slot t of the staged input = frame g(k, t), a copy of the bits.  Clips n_windows .. B - 1 repeat the
 *            last window's slot row (and fold nothing).
 *   FORWARD  exactly p3d_video_predict's pass.
 *   SCATTER  p3d_video_predict's NEWEST / MEAN rules with "t = 0 .. T - 1" replaced by "t = 0 .. live(k) - 1": one launch, k
 *            ascending, no atomics, the same laws for the counts; last_start = starts[n_windows - 1].  p3d_video_last_ms reports this
 *            call's gather and scatter.  The call returns synchronised.
 * Refused (-1, p3d_last_error names the first offender, nothing is launched and nothing changes): no open video; no table;
 * n_windows outside 1 .. B; then per window, in this order: a start outside [0, F - 1]; not ascending; a start that is neither its
 * shot's first frame nor T - 1 frames from its end (the message names the shot's [lo, hi]); a frame g(k, t) never put (the message
 * names the window and the first such slot's frame).
 * Calls of p3d_video_predict and p3d_video_predict_shots may be mixed on one video: they share the stores and last_start.  Under a
 * table of one shot the call returns p3d_video_predict's results bit for bit (the gather kernel differs: a slot at a time).
 * Example: F = 41, table 0 20 25 26 28 (shots of 20, 5, 1, 2, 13 frames).  Start 20 reads 20 21 22 23 24 23 22 21 20 21 22 23 24 23 22 21,
 * live 5; start 25 reads frame 25 sixteen times, live 1; start 26 reads 26 27 26 27 ..., live 2; start 28 reads 28 .. 40 39 38 37, live 13.
 * TEST HOOKS (tests/test_gpu_video_shot_windows.py, tests/test_shot_windows_cpu.py), under the table shot_starts [n_shots], validated as
 * p3d_video_set_shots validates it, with every frame counting as put:
 *   gather_slots   store [F][frame_elems] -> x [B][T][frame_elems] by GATHER (last_start -1), buffers and offset as p3d_debug_video_gather;
 *   scatter_shots  p3d_debug_video_scatter with LIVE: pred [B][T][hw][ld], store and count in place, device counts == plan counts;
 *   plan_shots     host only, no HIP call: the counts after the call in count_out [F], g in slots_out [B][T] (the padding clips'
 *                  rows included) and live_out [B] (0 for a padding clip); all three untouched after a refusal. */
int p3d_video_predict_shots(p3d_handle* h, const int* starts, int n_windows);
int p3d_debug_video_gather_slots(int device, const float* store, int F, int T, int64_t frame_elems, const int32_t* shot_starts, int n_shots,
                                 const int* starts, int n_windows, int B, int offset, float* x);
int p3d_debug_video_scatter_shots(int device, int mode, const float* pred, int B, int T, int64_t hw, int ld, const int32_t* shot_starts,
                                  int n_shots, const int* starts, int n_windows, int F, int last_start, float* store /* in/out [F][hw] */,
                                  int32_t* count /* in/out [F] */, int offset);
int p3d_debug_video_plan_shots(int mode, int F, int T, int B, int last_start, const int32_t* count_in, const int32_t* shot_starts, int n_shots,
                               const int* starts, int n_windows, int32_t* count_out, int* slots_out /* [B*T] */, int* live_out /* [B] */);

/* CRC-32C of a host buffer (host-side helper of the TensorFlow checkpoint reader / writer, sap3d_tensorflow_amd/tf_checkpoint.py:
 * the bundle format of train.py:180-185,266-267 checksums every tensor); crc = running value, 0 to start. */
uint32_t p3d_crc32c(const void* data, size_t n, uint32_t crc);

/* Releases every process-wide device resource of the library (scratch pools, the zero page) and synchronises the
 * device; live handles must be destroyed first.  The Python shim calls it from an atexit hook so that nothing of the
 * library is left for static destructors that may run after the HIP runtime is gone. */
int p3d_shutdown(void);

#ifdef __cplusplus
}
#endif
#endif
