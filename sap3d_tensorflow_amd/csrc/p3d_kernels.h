// Internal kernel-launch interface of libp3dhip (gfx950 only).
//
// Every convolution-like op of the P3D path (tf.nn.conv3d, its two gradients and
// tf.layers.conv3d_transpose, reference p3d.py:18-27,86,112,125,172,200-217) is
// expressed on ONE geometry: a "dense side" (the SAME conv's output lattice) and
// a "gathered side" (the conv's input lattice, reached through kernel taps).
//   conv forward      : iterate dense side,   gather input  at  g*s + (k - pad)
//   conv dgrad/deconv : iterate one residue class of the input lattice
//                       i = g*s + p, gather dense side at g + (p + pad - k)/s
//   conv wgrad        : reduce over the dense side, X gathered, dY dense
// so a launch is described by an iteration grid, per-tap integer offsets and an
// affine output map.  Layout is NDHWC with an explicit row stride (floats per
// position) so channel slices of concat buffers are addressed in place.
#pragma once
#include <vector>
#include <hip/hip_runtime.h>
#include <stdint.h>

#define P3D_MAX_TAPS 27
#ifndef P3D_WGRAD_GROUP
#define P3D_WGRAD_GROUP 6     // weight-gradient problems one grouped launch can carry (kernel-argument space)
#endif
#define P3D_STAT_REPLICAS 16   // lanes that share a channel's partial sums in the finalize kernels (fixed 4-step shuffle fold)
#define P3D_FOLD_MAX 32        // fused BatchNorm: up to this many per-tile partials a consuming launch folds itself (else a finalize launch)

// Tuning / diagnostic switches are environment variables only in a -DP3D_TUNING build (tools/*.sh pass it through
// P3D_EXTRA_HIPCC_FLAGS); in the product build they are absent, so a stray variable cannot change results or drop work.
#include <stdlib.h>
inline const char* p3d_tune_env(const char* name) {
#if defined(P3D_TUNING)
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

// Division by a launch-invariant extent without the ~40-instruction udiv expansion (the kernels' prologues decode linear
// positions into lattice coordinates): q = floor(n / d) for 0 <= n < 2^31 as mulhi(n, mul) >> shift with
// mul = ceil(2^(31+l) / d), l = ceil(log2 d) (Granlund & Montgomery, "Division by invariant integers", Thm 4.2); d = 1: mul = 0.
// (Measured: no change of any launch time -- the divisions sat in the shadow of the first loads -- kept for the shorter code.)
struct P3dFastDiv { unsigned mul; int shift; };
inline P3dFastDiv p3d_fastdiv(unsigned d) {
    P3dFastDiv f{0u, 0};
    if (d <= 1) return f;
    int l = 0;
    while ((1u << l) < d) ++l;
    f.mul = (unsigned)((((unsigned long long)1 << (31 + l)) + d - 1) / d);
    f.shift = l - 1;
    return f;
}
#if defined(__HIPCC__)
__device__ __forceinline__ unsigned p3d_div(unsigned n, P3dFastDiv f) { return f.mul ? (__umulhi(n, f.mul) >> f.shift) : n; }
#endif

// Wave priority of the kernels on the latency-bound main-stream chain.  The filter-gradient kernels that share the chip with
// them from the side stream stay at priority 0, so a SIMD that hosts both issues the chain's instructions first: the chain
// is what the step waits for, the filter gradients only have to be done by the end (measured: 17.13 -> 16.66 ms per step,
// priority 1 and 3 alike; profiles/r03_prio_ab.json).
#if defined(__HIPCC__)
#define P3D_CHAIN_PRIO() __builtin_amdgcn_s_setprio(2)
// Kernel arguments arrive through the scalar cache, one 64-byte line per first touch, and hipcc reads them where they are used:
// a kernel with a 1 KB argument struct walks into one cold line after another (measured: 13 dependent s_load / s_waitcnt round
// trips, 2.3 us, between the entry of the pipelined conv kernel and its first operand load).  Touch every line of the struct
// at entry, all loads in flight together: one miss latency, and what follows hits the cache.
// ONE asm statement per kernel, the wait inside it: scalar loads return out of order and hipcc does not count an asm statement's
// loads, so a load still in flight behind the statement could land in a register the compiler has meanwhile given to
// something else (it did: wrong convolutions).  All loads of the statement target the same scratch SGPR.
typedef const unsigned __attribute__((address_space(4))) p3d_karg_t;
#define P3D_WL(off) "s_load_dword %0, %1, " #off "\n\t"
#define P3D_WL4(a, b, c, d) P3D_WL(a) P3D_WL(b) P3D_WL(c) P3D_WL(d)
template <int LINES>
__device__ __forceinline__ void p3d_warm_kernarg_lines() {
    p3d_karg_t* ka = (p3d_karg_t*)__builtin_amdgcn_kernarg_segment_ptr();
    unsigned t;
    // the largest supported count that stays inside the struct (never a load past the arguments)
    if constexpr (LINES >= 17)
        asm volatile(P3D_WL4(0x0, 0x40, 0x80, 0xc0) P3D_WL4(0x100, 0x140, 0x180, 0x1c0) P3D_WL4(0x200, 0x240, 0x280, 0x2c0)
                     P3D_WL4(0x300, 0x340, 0x380, 0x3c0) P3D_WL(0x400) "s_waitcnt lgkmcnt(0)" : "=&s"(t) : "s"(ka) : "memory");
    else if constexpr (LINES >= 14)
        asm volatile(P3D_WL4(0x0, 0x40, 0x80, 0xc0) P3D_WL4(0x100, 0x140, 0x180, 0x1c0) P3D_WL4(0x200, 0x240, 0x280, 0x2c0)
                     P3D_WL(0x300) P3D_WL(0x340) "s_waitcnt lgkmcnt(0)" : "=&s"(t) : "s"(ka) : "memory");
    else if constexpr (LINES >= 11)
        asm volatile(P3D_WL4(0x0, 0x40, 0x80, 0xc0) P3D_WL4(0x100, 0x140, 0x180, 0x1c0) P3D_WL(0x200) P3D_WL(0x240) P3D_WL(0x280)
                     "s_waitcnt lgkmcnt(0)" : "=&s"(t) : "s"(ka) : "memory");
    else if constexpr (LINES >= 8)
        asm volatile(P3D_WL4(0x0, 0x40, 0x80, 0xc0) P3D_WL4(0x100, 0x140, 0x180, 0x1c0) "s_waitcnt lgkmcnt(0)" : "=&s"(t) : "s"(ka) : "memory");
    else if constexpr (LINES >= 6)
        asm volatile(P3D_WL4(0x0, 0x40, 0x80, 0xc0) P3D_WL(0x100) P3D_WL(0x140) "s_waitcnt lgkmcnt(0)" : "=&s"(t) : "s"(ka) : "memory");
    else if constexpr (LINES >= 4)
        asm volatile(P3D_WL4(0x0, 0x40, 0x80, 0xc0) "s_waitcnt lgkmcnt(0)" : "=&s"(t) : "s"(ka) : "memory");
    else if constexpr (LINES >= 2)
        asm volatile(P3D_WL(0x0) P3D_WL(0x40) "s_waitcnt lgkmcnt(0)" : "=&s"(t) : "s"(ka) : "memory");
}
template <class Args>
__device__ __forceinline__ void p3d_warm_kernargs() { p3d_warm_kernarg_lines<(int)((sizeof(Args) + 63) / 64)>(); }
#endif

struct P3dTap {
    int16_t dd, dh, dw;   // gathered coordinate = g*is + d{d,h,w}
    int16_t widx;         // which [K][N] slab of the weight tensor
};

// ---- BatchNorm fused into the convolutions' operand paths (reference p3d.py:56-81,88-97: every bn -> relu pair
//      between two convs of a bottleneck) ---------------------------------------------------------------------------
// The normalised tensor is never stored: the conv that consumes it reads the RAW output y of the producing conv and
// applies  relu(scale*y + shift)  to its A fragments between LDS and the matrix cores; the per-channel (scale, shift)
// come from the producer's per-tile statistics partials, folded in the consumer's prologue (few partials) or by a
// finalize launch (many).  Backward mirrors it: an input-gradient launch gates its result with the ReLU mask of the
// BatchNorm OUTPUT it differentiates through and leaves per-tile (sum g, sum g*xhat); the next input-gradient launch
// (and the filter gradients) read  dy = k1*g + k2*y + k3  on their operand path.
struct BnFold {            // forward: (scale, shift) of one BatchNorm over C channels
    const float* gamma; const float* beta;
    const float* part; int nparts;               // producer's (sum, sumsq) partials [nparts][C][2]; null: read scale / shift below
    int C;
    float* scale; float* shift; float* mean; float* invstd;     // written by block 0 when `publish` (else read when part == null)
    float* moving_mean; float* moving_var;       // momentum-0.99 update by the publisher when update_moving
    double inv_m;                                // 1 / rows of the normalised tensor
    float eps; int publish; int update_moving;
};
struct BnGradFold {        // backward: dy = k1*g + k2*y + k3  (g: gated gradient of the BN output, y: BN input)
    const float* gamma; const float* mean; const float* invstd;
    const float* part; int nparts;               // (sum g, sum g*xhat) partials [nparts][C][2]; null: read coef below
    int C;
    float* coef;                                 // [3][C] k1, k2, k3: written by block 0 when `publish`, read by the filter gradients
    float* dgamma; float* dbeta;                 // BN parameter gradients, written by the publisher
    double inv_m; int publish;
};
struct BnGate {            // epilogue of an input-gradient launch: g = (scale*y + shift > 0) ? v : 0
    const float* y; int ldy;                     // the BN's input (a conv output) on this launch's output lattice
    const float* scale; const float* shift; const float* mean; const float* invstd;
    float* out; int ldo;                         // gated gradient
    float* part;                                 // [m tiles][Nc][2]  (sum g, sum g*xhat) per output-tile row, plain stores
};
enum { P3D_AT_NONE = 0, P3D_AT_RELU1 = 1, P3D_AT_RELU2 = 2, P3D_AT_GRAD = 3 };
//  RELU1: a = relu(s1*x + t1)                           RELU2: a = relu(s1*x + t1) + relu(s2*x2 + t2)   (ST_B / ST_C sums)
//  GRAD : a = k1*x + k2*x2 + k3   (x = gated gradient, x2 = BN input); padded taps stay 0

// Implicit-GEMM convolution launch:  Y[m, n] (+)= sum_taps sum_k A[m+tap, k] * B_tap[k, n] (+ bias[n])
struct IgemmArgs {
    const float* x;       // gathered operand (already offset to its channel slice)
    int N, Di, Hi, Wi;    // gathered-side extents
    int ldx;              // floats per gathered-side position
    int K;                // reduction channels (Cin of this GEMM)
    int Gd, Gh, Gw;       // iteration grid per sample; M = N*Gd*Gh*Gw
    P3dFastDiv fGd, fGh, fGw;   // (filled by the launcher)
    int isd, ish, isw;    // gathered coord = g*is + tap offset
    float* y;             // output (already offset to its channel slice)
    int Do, Ho, Wo;       // output extents
    int ldy;              // floats per output position
    int Nc;               // output channels of this GEMM
    int osd, osh, osw, ood, ooh, oow;   // output coord = g*os + oo
    const float* w;       // weights: slab widx is [K][Nc] (wT=0) or [Nc][K] (wT=1)
    int wT;
    const float* bias;    // [Nc] or null
    // BatchNorm statistics epilogue: per-(output tile row, channel) partial (sum, sum of squares) of the stored values,
    // written with plain stores to statpart[(stat_base + m_tile) * Nc + col][2] -- no atomics, so the statistics (and
    // everything downstream) are bit-reproducible; p3d_bn_finalize folds the partials in a fixed order.  Null: none.
    float* statpart;
    int stat_base;
    int accum;            // 1: Y += result (gradient accumulation)
    const float* zeros;   // >= 128 B of zeros in device memory (source for padded / tail lanes)
    // K-slicing (filled by the launcher from the plan): slice s of a tile stores its partial tile to
    // slab[(tile * nsplit + s) * BM*BN], the block whose arrival ticket is the last one sums the slices in slice order
    // (bit-reproducible, unlike atomics), applies bias / accumulate / statistics and writes the output.
    float* slab; unsigned* cnt; int nsplit;
    int f16;              // 1: round the operand fragments to fp16 and use the fp16 MFMA (fp32 accumulate); pointwise convs of configs[4]
    int xcd_min_tiles;    // set by the launcher: launches / classes with at least this many tiles map consecutive tiles to one XCD
    // fused BatchNorm on the A operand (P3D_AT_*): x2 is the second source on the gathered lattice (RELU2, GRAD)
    int at_mode;
    const float* x2; int ldx2;
    BnFold f1, f2;        // RELU1 / RELU2: the BatchNorms of x and x2
    BnGradFold gf;        // GRAD
    // gated epilogue (input gradients through a fused BatchNorm + ReLU): the value v of every output element
    // (after bias / accumulate) goes raw to y when raw_store, and gated to gate[q].out; ngate = 0: plain store to y
    int ngate, raw_store;
    BnGate gate[2];
    int ntaps;
    P3dTap taps[P3D_MAX_TAPS];
};

// What differs between the launches of one group -- the residue classes of a transposed conv / of a strided conv's input
// gradient: iteration grid, output offset, kernel taps.  One grouped launch carries all of them (p3d_launch_igemm2_group):
// a class alone offers too few tiles for 256 CUs (deconv3 at 8 clips: 196 tiles of 128x128 per class, eight classes).
#define P3D_IGEMM_CLASSES 8
struct IgemmClass {
    int Gd, Gh, Gw;
    P3dFastDiv fGd, fGh, fGw;
    int ood, ooh, oow;
    int stat_base;        // first statistics partial of this class (its m tiles follow each other)
    int ntaps;
    int blk0;             // first block of this class in the grouped launch (classes in descending order of work)
    const float* w; const float* bias; float* y; float* statpart;      // per class as well: sibling convs on one input (ST_B)
    int nsplit;           // K-slices of this class (its blocks: tiles x slices, a tile's slices in consecutive blocks)
    int tile0;            // first output tile of this class in its grid (> 0: the K-sliced tail of the class before it)
    int ntiles;           // output tiles of this class
    long long slab0, cnt0;      // this class's share of the launch's slab / counter scratch (floats / counters)
    P3dTap taps[P3D_MAX_TAPS];
};
struct IgemmGroupArgs {
    IgemmArgs common;     // everything the classes share (its own grid / offsets / taps are unused)
    int nclass;
    IgemmClass cls[P3D_IGEMM_CLASSES];
};

// Tile and split-K choice of the pipelined kernel (conv_igemm2.hip)
struct P3dIgemmPlan {
    int bm = 64, bn = 64, splits = 1;
    const char* name = "";
    int stream_blocks = 0;      // > 0: the launch runs on the weights-resident streaming kernel (conv_pointwise.hip) with this many blocks
};
// number of output-tile rows (= statistics partials) a launch with this plan produces
inline int p3d_igemm2_mtiles(const IgemmArgs& a, const P3dIgemmPlan& pl) {
    if (pl.stream_blocks > 0) return pl.stream_blocks;      // one statistics partial per block
    const long long M = (long long)a.N * a.Gd * a.Gh * a.Gw;
    return (int)((M + pl.bm - 1) / pl.bm);
}
// Per-stream scratch for K-sliced launches (partial tiles + arrival counters).  Launches on one stream run in order, so
// they share it; the buffers only grow, and an outgrown buffer stays allocated (captured graphs may still name it).
hipError_t p3d_stream_scratch(hipStream_t s, size_t slab_floats, size_t counters, float** slab, unsigned** cnt);
long long p3d_scratch_dirty_counters();      // test hook: non-zero arrival counters with nothing in flight (must be 0)
void p3d_release_scratch();     // frees every scratch buffer (process shutdown; no launch may be in flight)

// Weight-gradient launch: dW[widx][k][n] += sum_m Xg[m+tap, k] * dY[m, n]
struct WgradArgs {
    const float* x;       // gathered operand (conv input side)
    int N, Di, Hi, Wi, ldx, K;
    int Gd, Gh, Gw;       // dense grid (conv output side); M = N*Gd*Gh*Gw
    int isd, ish, isw;
    const float* dy;      // dense operand
    int ldy, Nc;
    float* dw;            // [slab][K][Nc]; the launch ADDS the gradient to it (single writer per element: plain read-modify-write)
    float* dbias;         // [Nc] or null (column sums of dy, added by tap 0 / k-tile 0 blocks)
    int ksplit;           // (chosen by the launcher)
    int greedy;           // 1: launched when nothing else is running -- take every LDS slot (conv_wgrad2.hip, launch_group_t)
    int polite;           // 1: runs beside a chain of small launches whatever its own size -- one block per CU
    int pair;             // 1 (K <= 32): two taps share a 64-row tile (the stem's 28-float kernel rows)
    const float* zeros;   // zero page
    // fused BatchNorm: operand transforms with per-channel coefficients the forward / the input-gradient launches published
    int xt;               // gathered operand: 0 plain, 1 relu(xs1*x + xt1), 2 relu(xs1*x + xt1) + relu(xs2*x2 + xt2)
    const float* x2; int ldx2;
    const float* xs1; const float* xt1; const float* xs2; const float* xt2;     // [K]
    int dyt;              // dense operand: 0 plain, 1 dcoef[0][n]*dy + dcoef[1][n]*dy2 + dcoef[2][n]
    const float* dy2; int ldy2;
    const float* dcoef;   // [3][Nc]
    int ntaps;
    P3dTap taps[P3D_MAX_TAPS];
};

#ifdef __cplusplus
extern "C++" {
#endif

P3dIgemmPlan p3d_igemm2_plan(const IgemmArgs& a, int allow_split);
// Autotuning window (graph build): inside it, the first plan request for a new shape is decided by timing the
// candidates on stream `s` with the caller's real buffers; outside it, a heuristic answers for unseen shapes.
void p3d_tune_begin(hipStream_t s);
void p3d_tune_end();
hipError_t p3d_launch_igemm2(const IgemmArgs& a, const P3dIgemmPlan& plan, hipStream_t s);
// n launches that differ only in what IgemmClass holds, as ONE launch (same tile shape, no operand transform / gates; n <= 8).
// stat_base of every class must be set by the caller (statistics partials of class q start at its stat_base).
bool p3d_igemm2_tail_split(const IgemmArgs& a, const P3dIgemmPlan& pl);      // a single launch whose last round gets K-sliced (goes out grouped)
bool p3d_igemm2_groupable(const IgemmArgs* v, int n, const P3dIgemmPlan& plan);
hipError_t p3d_launch_igemm2_group(const IgemmArgs* v, int n, const P3dIgemmPlan& plan, hipStream_t s);
void p3d_igemm2_override(int tile, int splits);   // test / tools hook: force the tile (0: 64x64, 1: 128x64, 2: 128x128) and the K-slice count; -1 / 0 = no override
// dense 1x1x1 convs over >= 16 384 positions with K * N <= 16 384 (conv_pointwise.hip): 0 = not that case, else the block count
int p3d_pw_stream_blocks(const IgemmArgs& a);
int p3d_pw_stream_max_blocks(long long M, int N);      // upper bound of p3d_pw_stream_blocks over every launch with an M x N output
hipError_t p3d_launch_pw_stream(const IgemmArgs& a, hipStream_t s);
hipError_t p3d_launch_wgrad2(const WgradArgs& a, hipStream_t s);
hipError_t p3d_launch_wgrad2_group(const WgradArgs* probs, int n, hipStream_t s);   // up to P3D_WGRAD_GROUP problems, one launch
const char* p3d_wgrad2_variant(const WgradArgs& a);
const char* p3d_wgrad2_group_variant(const WgradArgs* probs, int n, bool fused);      // the label of a grouped launch (its tile)
// test hook (host only): cuts[i] of problem i in that launch (0: dropped), the slab stride, the tile; returns the live problems or -1
int p3d_wgrad2_group_cuts(const WgradArgs* probs, int n, int* cuts, int* kstride, int* tm, int* tn);
void p3d_wgrad2_force_tile(int tm, int tn);      // test hook: tile of single-problem launches (64 / 128 each); 0, 0 = the plan's choice

// ---- BatchNorm (tf.layers.batch_normalization, rank-5, eps 1e-3) ------------------------------
struct BnParams {          // device pointers, all [C]
    const float* gamma; const float* beta;
    float* moving_mean; float* moving_var;
    const float* statpart; // [nparts][C][2] partial (sum, sumsq) written by the producer's epilogue or p3d_bn_stats
    int nparts;
    float* scale; float* shift;      // y_hat = scale*y + shift
    float* mean; float* invstd;      // saved for backward
    int C;
};
// use_batch: statistics from `stats` over M rows, else moving stats.  update_moving: momentum 0.99 update.
hipError_t p3d_bn_finalize(const BnParams& bn, long M, int use_batch, int update_moving, float eps, hipStream_t s);
// statpart[b][c] = (sum, sum of squares) over block b's rows of y, b < p3d_bn_stats_parts(M, C)
// (for producers that cannot do it in their epilogue)
int p3d_bn_stats_parts(long M, int C);
hipError_t p3d_bn_stats(const float* y, int ld, long M, int C, float* statpart, hipStream_t s);

// coefficients of a fused BatchNorm's backward from many partials (few: the consuming launch folds them itself)
hipError_t p3d_bn_grad_finalize(const BnGradFold& f, hipStream_t s);

// Fused normalise/activate/add passes.  Modes (reference p3d.py lines in brackets):
//  0: z = relu(bn1(y1))                         [58-59, 88+97, 173-174, 201-202]
//  1: z = relu(bn1(y1) + r)                     [114,133-134 identity residual]
//  2: z = relu(bn1(y1) + bn2(y2))               [114,127,133-134 projected residual]
//  3: z = relu(bn1(y1)) + relu(bn2(y2))         [ST_B 65-72]
//  4: z = r + relu(bn1(y1))                     [ST_C 74-81]
struct BnApplyArgs {
    int mode;
    long M; int C;
    const float* y1; int ld1; const float* scale1; const float* shift1;
    const float* y2; int ld2; const float* scale2; const float* shift2;   // y2 doubles as r (modes 1,4)
    float* z; int ldz;
    float drop_scale;      // >0: inverted dropout with this keep scale (p3d.py:214), keyed by seed
    float drop_rate; unsigned long long seed;
    const unsigned long long* seed_dev;   // non-null: the seed is read from device memory (captured step graphs)
};
hipError_t p3d_bn_apply(const BnApplyArgs& a, hipStream_t s);
// finalize + apply in one launch when every block can fold its own 64 channels' partials (<= 128 per BN, no dropout)
bool p3d_bn_fold_apply_ok(long M, int C, int nparts1, int nparts2, float drop_scale);
hipError_t p3d_bn_fold_apply(const BnApplyArgs& a, const BnParams& bn1, const BnParams& bn2, int batch1, int batch2, int update_moving,
                             float eps, hipStream_t s);

// Backward of the passes above.  Pass 1 reduces per channel sum(dz') and sum(dz' * xhat) into per-block
// partials part1/part2; a finalize pass folds them in block order into coef1/coef2 ([C][2] floats: the two sums / M) and the parameter gradients; pass 2
// writes the input gradients.
struct BnBwdArgs {
    int mode;
    long M; int C;
    const float* dz; int lddz;
    const float* y1; int ld1; const float* scale1; const float* shift1; const float* mean1; const float* invstd1;
    const float* y2; int ld2; const float* scale2; const float* shift2; const float* mean2; const float* invstd2;
    const float* gamma1; const float* gamma2;
    float* part1; float* part2;      // per-block partial sums [nparts][C][2] (plain stores: no atomics), nparts = p3d_bn_bwd_parts(M, C)
    int nparts;
    float* coef1; float* coef2;
    float* dgamma1; float* dbeta1; float* dgamma2; float* dbeta2;      // parameter grads (written)
    int batch1, batch2;    // 1: batch statistics were used (full BN backward), 0: inference BN
    float* dy1; int lddy1; int acc1;
    float* dy2; int lddy2; int acc2;      // dy2 doubles as dr (modes 1,4)
    float drop_scale; float drop_rate; unsigned long long seed; const unsigned long long* seed_dev;
};
int p3d_bn_bwd_parts(long M, int C);
hipError_t p3d_bn_bwd_reduce(const BnBwdArgs& a, hipStream_t s);
hipError_t p3d_bn_bwd_finalize(const BnBwdArgs& a, hipStream_t s);
hipError_t p3d_bn_bwd_apply(const BnBwdArgs& a, hipStream_t s);

// Small-tensor BatchNorm (bn_small.hip): one launch forward, one launch backward, M <= 1024 rows.
struct BnSmallArgs {
    int mode; int M; int C;
    const float* y1; int ld1;
    const float* y2; int ld2;           // second BN input (modes 2,3) or residual (modes 1,4)
    BnParams bn1, bn2;
    int batch1, batch2;                 // 1: batch statistics, 0: moving statistics
    int update_moving; float eps;
    float* z; int ldz;
    const float* dz; int lddz;          // backward
    float* dy1; int lddy1;
    float* dy2; int lddy2; int acc2;
    float* dgamma1; float* dbeta1; float* dgamma2; float* dbeta2;
};
bool p3d_bn_small_ok(long M, int C);
hipError_t p3d_bn_small_fwd(const BnSmallArgs& a, hipStream_t s);
hipError_t p3d_bn_small_bwd(const BnSmallArgs& a, hipStream_t s);

// ---- GroupNorm (gn.hip; reference gn/p3d_gn.py:24-46).  Tables are indexed [n*C + c]. -------------------
struct GnParams {
    const float* gamma; const float* beta;       // [C]
    double* sums;                                // [N][C][2]: forward (sum, sumsq) or backward (sum g, sum g*xhat)
    float* scale; float* shift; float* mean; float* invstd;     // [N][C]
    float* coef;                                 // [N][C][3] backward coefficients (k, c1, c2)
    int C, G;
};
struct GnApplyArgs {
    int mode;                                    // 0,1,3,4,5,6 (gn.hip header)
    long M; int R; int C;                        // M = N*R rows, R rows per sample
    const float* y1; int ld1; GnParams g1;
    const float* y2; int ld2; GnParams g2;       // second GN input (mode 3) or residual / CBAM input (1,4,6)
    const float* cs; const float* ss;            // mode 6: CBAM channel scale [N][C], spatial scale [M]
    float* z; int ldz;
    const float* dz;                             // backward: gradient of z (same stride as z)
    float* dy1; int lddy1;
    float* dy2; int lddy2; int acc2;             // mode 3: GN2 input grad; 1,4: residual grad; 6: grad of the CBAM output
    float drop_scale; float drop_rate; unsigned long long seed; const unsigned long long* seed_dev;
    // epsilon of the one-launch path for small tensors (p3d_gn_small_*), and where its parameter gradients are STORED
    float eps; float* dgamma1; float* dbeta1; float* dgamma2; float* dbeta2;
    float* part; unsigned* counters;             // backward partial sums + arrival counters (set by the launchers)
};
bool p3d_gn_small_ok(int R, int C, int G);       // a (sample, group) slab fits one block's registers
hipError_t p3d_gn_small_fwd(const GnApplyArgs& a, hipStream_t s);    // stats + tables + normalise/activate in one launch
hipError_t p3d_gn_small_bwd(const GnApplyArgs& a, hipStream_t s);    // whole backward in one launch
hipError_t p3d_gn_stats(const float* y, int ld, int N, int R, int C, double* sums, hipStream_t s);
hipError_t p3d_gn_finalize(const GnParams& p, int N, int R, float eps, hipStream_t s);
hipError_t p3d_gn_apply(const GnApplyArgs& a, hipStream_t s);
hipError_t p3d_gn_bwd_reduce(const GnApplyArgs& a, hipStream_t s);
hipError_t p3d_gn_bwd_finalize(const GnParams& p, int N, int R, float* dgamma, float* dbeta, hipStream_t s);
hipError_t p3d_gn_bwd_apply(const GnApplyArgs& a, hipStream_t s);

// ---- CBAM (cbam.hip; reference utils/network.py:198-274 as used at gn/p3d_gn.py:175) --------------------
struct CbamArgs {
    const float* x; int ld;                      // block residual [N, D,H,W, C]
    int N, D, H, W, C, Ch;                       // Ch = C / 8 hidden units
    const float* k0; const float* b0; const float* k1; const float* b1;     // shared MLP  C->Ch->C
    const float* k7;                             // [7,7,7,2,1]
    int chunks;                                  // row chunks per sample of the pooling / backward passes
    float* part;                                 // [N][chunks][C][3] partial (sum, max, ties-of-max)
    float* avg; float* mx; float* ties;          // [N][C]
    float* havg; float* hmx;                     // [N][Ch] post-ReLU hidden activations
    float* cs;                                   // [N][C]   channel scale = sigmoid(mlp(avg) + mlp(max))
    float* sp;                                   // [M][2]   channel-mean / channel-max of x*cs
    float* ss;                                   // [M]      spatial scale = sigmoid(conv7(sp))
    // backward
    const float* dout;                           // [M][C] gradient of the CBAM output (dense)
    float* dpre;                                 // [M]
    float* dsp;                                  // [M][2]
    float* dcs_part;                             // [N][chunks][C]
    float* dO;                                   // [N][C] gradient of the MLP output (pre-sigmoid)
    float* davg; float* dmx;                     // [N][C] gradients of the pooled vectors
    float* dh;                                   // [N][2][Ch] gradients of the hidden activations (avg, max branch)
    float* dx; int lddx; int accx;               // gradient of x
    float* dk0; float* db0; float* dk1; float* db1; float* dk7;
    float* k7part; unsigned* k7counter;          // dK7 partials [blocks][343][2] + arrival counter (set by the launcher)
};
hipError_t p3d_cbam_forward(const CbamArgs& a, hipStream_t s);
hipError_t p3d_cbam_backward(const CbamArgs& a, hipStream_t s);

// ---- self attention (attention.hip; reference utils/network.py:157-192) -----------------------------------
hipError_t p3d_softmax_rows(float* s, long long rows, int cols, int ld, hipStream_t st);          // in place; columns [cols, ld) := 0
hipError_t p3d_softmax_rows_bwd(const float* beta, float* d, long long rows, int cols, int ld, hipStream_t st);   // d := ds, in place
struct AttnMixArgs {                 // z = r * gamma + x  (utils/network.py:191), optional dropout on z (p3d.py:388)
    long long M; int C;
    const float* r; int ldr;         // relu(bn(conv(o)))
    const float* x; int ldx;         // the block's input
    const float* gamma;              // [1]
    float* z; int ldz;
    float drop_scale; float drop_rate; unsigned long long seed; const unsigned long long* seed_dev;
    // backward
    const float* dz; float* dr; float* dx; int accx; float* dgamma;
    float* part; unsigned* counter;  // dgamma partials per block + arrival counter (set by the launcher)
};
hipError_t p3d_attn_mix_fwd(const AttnMixArgs& a, hipStream_t s);
hipError_t p3d_attn_mix_bwd(const AttnMixArgs& a, hipStream_t s);
// The attention core  o = softmax(g f^T) h  (utils/network.py:183-185) without the score matrix in HBM (attention_flash.hip):
// per clip, g [Ng x ch/8] queries, f [Nf x ch/8] keys, h [Nf x ch] values; clip b of a tensor starts b * rows * ld floats in.
struct FlashAttnArgs {
    int B, Ng, Nf, ch;                   // ch in {32, 64, 128, 256}; ch/8 channels in g and f
    const float* g; int ldg;
    const float* f; int ldf;
    const float* h; int ldh;
    float* o; int ldo;                   // forward output [B][Ng][ch]
    float* lse;                          // [B][Ng]: row maximum + log of the row sum (kept for the backward pass)
    // backward
    const float* d_o; int lddo;          // gradient of o
    float* dsum;                         // [B][Ng] scratch: <d_o, o> per row
    float* dg; int lddg; float* df; int lddf; float* dh; int lddh;       // written, not accumulated
};
bool p3d_flash_attn_ok(int ch);
hipError_t p3d_flash_attn_fwd(const FlashAttnArgs& a, hipStream_t s);
hipError_t p3d_flash_attn_bwd(const FlashAttnArgs& a, hipStream_t s);      // three launches: row dots, dg, (df, dh)
hipError_t p3d_pad_rows(const float* src, float* dst, int B, int N, int Npad, int C, hipStream_t s);     // [B][N][C] -> [B][Npad][C], zero tail
hipError_t p3d_unpad_rows(const float* src, float* dst, int B, int N, int Npad, int C, hipStream_t s);   // the reverse (tail dropped)

// ---- max pool (tf.nn.max_pool3d SAME; p3d.py:177,183,189,195) ---------------------------------
struct PoolArgs {
    const float* x; int N, Di, Hi, Wi, C, ldx;
    float* y; int Do, Ho, Wo, ldy;
    int kd, kh, kw, sd, sh, sw, pd, ph, pw;
    // backward
    const float* dy; int lddy; float* dx; int lddx;
    unsigned* idx;       // optional [N*Do*Ho*Wo][C/4] words, one byte per channel: tap (kd,kh,kw scan order) of the
                         // first maximum; written by the forward, read by p3d_maxpool_bwd_gather
};
hipError_t p3d_maxpool_fwd(const PoolArgs& a, hipStream_t s);
// overlapping windows without atomics or a zero fill: every input cell collects from the (few) windows that contain it,
// using the arg-max taps the forward stored.  Writes dx, or adds to it (accumulate = 1).
hipError_t p3d_maxpool_bwd_gather(const PoolArgs& a, int accumulate, hipStream_t s);
bool p3d_maxpool_disjoint(const PoolArgs& a);                    // k == s, no padding: windows do not overlap
hipError_t p3d_maxpool_bwd_disjoint(const PoolArgs& a, int accumulate, hipStream_t s);   // writes / accumulates dx, no atomics

// ---- output head: tf.layers.conv3d_transpose(x, 1, 3, 2, 'same') + sigmoid (p3d.py:217-219) ---
struct HeadArgs {
    const float* x; int N, D, H, W, C;     // input [N,D,H,W,C], output [N,2D,2H,2W,1]
    const float* k;                        // kernel [3,3,3,1,C]
    const float* bias;                     // [1]
    float* logits; float* pred;            // pre- and post-sigmoid
    int sigmoid;                           // 0: pred = logits (p3d_concat head, p3d.py:275)
    const float* dlogits; float* dx; float* dk; float* dbias;
    float* part; unsigned* counter;        // filter-gradient partials [blocks][28][C] + arrival counter (set by the launcher)
};
// path: P3D_HEAD_RULE = the launcher's own choice (what the network runs); a forced kernel the shape or alignment does not allow
// is hipErrorInvalidValue.  done (optional): the kernel that ran and its grid.
enum { P3D_HEAD_RULE = 0, P3D_HEAD_LANES = 1, P3D_HEAD_GENERIC = 2, P3D_HEAD_FILTER4 = 1, P3D_HEAD_FILTER1 = 2, P3D_HEAD_STRIDE1 = 3 };
struct HeadLaunch { int kernel; unsigned blocks; };
hipError_t p3d_head_fwd(const HeadArgs& a, hipStream_t s, int path = P3D_HEAD_RULE, HeadLaunch* done = nullptr);
hipError_t p3d_head_bwd_input(const HeadArgs& a, hipStream_t s);    // dx written
// dk, dbias += (per-block partials folded in block order; HEAD_FOLD blocks per group, then the groups, on the FILTER4 kernel)
hipError_t p3d_head_bwd_filter(const HeadArgs& a, hipStream_t s, int path = P3D_HEAD_RULE, HeadLaunch* done = nullptr);
// the stride-1 variant tf.layers.conv3d(x, 1, 3, 1, 'same') (gn/p3d_gn.py:537): D,H,W are both input and output extents
hipError_t p3d_headc_fwd(const HeadArgs& a, hipStream_t s, HeadLaunch* done = nullptr);
hipError_t p3d_headc_bwd_input(const HeadArgs& a, hipStream_t s);
hipError_t p3d_headc_bwd_filter(const HeadArgs& a, hipStream_t s, HeadLaunch* done = nullptr);

// What a launch list row says about one launch: the kernel's name and its flop / byte figures (bench.py's roofline).
struct LaunchDesc { const char* kernel; double flops, bytes; };

// ---- loss (p3d_set_loss kinds 0, 1, 2), fused with the gradient at the logits ----------------------------------
// *loss_out += the loss (a double accumulator; the network zeroes it first).  z = logits, p = pred, t = target:
//   kind 0, Smooth-L1 sum (utils/network.py:49-62, train.py:159): dlogits = dL/dpred, times pred*(1-pred) when through_sigmoid
//   kind 1, sigmoid cross-entropy on the logits: dlogits = sigmoid(z) - t (the stored pred when through_sigmoid)
//   kind 2, L1 sum (train.py:160): dlogits = sign(p - t), times pred*(1-pred) when through_sigmoid
// Smooth-L1 never reads the logits.  Any other kind: hipErrorInvalidValue.
struct LossArgs {
    int kind;
    const float* logits; const float* pred; const float* target;
    long n;
    int through_sigmoid;
    double* loss_out; float* dlogits;
};
LaunchDesc p3d_loss_desc(const LossArgs& a);
// done (optional): [0] = 1 float4 path (n % 4 == 0, every operand the kind uses 16-byte aligned), 2 scalar path; [1] = blocks
hipError_t p3d_loss(const LossArgs& a, hipStream_t s, unsigned* done = nullptr);

// ---- per-map saliency losses (map_loss.hip; p3d_set_loss P3D_LOSS_KLD_CC) ------------------------------------------------
// `maps` maps of N = map_elems consecutive elements; s = pred (through_sigmoid) or 1/(1+expf(-logits)).  Three stages in
// order on one stream: 0 sums, 1 terms (+= the weighted loss into *loss_out), 2 dlogits.  Scratch: p3d_map_loss_scratch's
// doubles and counters, the counters zero before the first launch (every stage leaves them zero).  mstat[m] holds
// S, Y, KL_m, CC_m (NaN where undefined), sum g p, A, B, C, the map's loss term.
constexpr int P3D_MAP_STATS = 10;
constexpr long long P3D_MAP_LOSS_ELEMS_PER_BLOCK = 2048;
struct MapLossArgs {
    const float* logits; const float* pred; const float* target;
    float* dlogits; double* loss_out;
    long long maps, N;
    int blocks;                  // per map: p3d_map_loss_blocks(N)
    int through_sigmoid, vec4;
    float kld_weight, cc_weight;
    double* mstat; double* part; unsigned* cnt;
};
int p3d_map_loss_blocks(long long map_elems);
void p3d_map_loss_scratch(long long maps, long long map_elems, size_t* doubles, size_t* counters);
MapLossArgs p3d_map_loss_args(const float* logits, const float* pred, const float* target, long long maps, long long map_elems,
                              int through_sigmoid, float kld_weight, float cc_weight, double* loss_out, float* dlogits,
                              double* scratch, unsigned* counters);
hipError_t p3d_map_loss_launch(int stage, const MapLossArgs& a, hipStream_t s);

// ---- the same with NSS and SIM terms and a fixation map (map_loss.hip; p3d_set_loss P3D_LOSS_SALIENCY) ------------------
// w_kld KL + w_cc (1 - CC) + w_nss (-NSS) + w_sim (1 - SIM) per map, in sibling kernels of the three above over the same grid
// (the P3D_LOSS_KLD_CC launches are untouched); m carries what they share.  fix: one byte per element, fixated <=> byte >= 128;
// read only when nss_weight > 0 (use_fix), four bytes at a time on the float4 path.  The KL and CC parts are the expressions of
// the kernels above, so with nss_weight = sim_weight = 0 loss and dlogits are theirs bit for bit.  Scratch:
// p3d_saliency_loss_scratch's doubles and counters (counters zero before the first launch, left zero).  m.mstat[m] as above;
// xstat[m] holds min s, max s, min y, max y, F, S_f, NSS_m, SIM_m (NaN where undefined), sum [p' < q'] p'.
constexpr int P3D_SAL_STATS = 10;
constexpr int P3D_SAL_PARTS = 8;      // partials per block: stage 0 writes eight, stage 1 seven
struct SaliencyLossArgs {
    MapLossArgs m;
    const unsigned char* fix;
    int use_fix;
    float nss_weight, sim_weight;
    double* xstat;
};
void p3d_saliency_loss_scratch(long long maps, long long map_elems, size_t* doubles, size_t* counters);
SaliencyLossArgs p3d_saliency_loss_args(const float* logits, const float* pred, const float* target, const unsigned char* fix,
                                        long long maps, long long map_elems, int through_sigmoid, float kld_weight, float cc_weight,
                                        float nss_weight, float sim_weight, double* loss_out, float* dlogits, double* scratch,
                                        unsigned* counters);
hipError_t p3d_saliency_loss_launch(int stage, const SaliencyLossArgs& a, hipStream_t s);

// ---- the optimiser step (p3d_set_optimizer), with or without regularisation (p3d_set_regularization) ---------------
// Regularisation: the flat range is cut at plan time into tiles, each with ONE float32 coefficient c (0 on undecayed variables
// and on slot padding).  off is relative to the table's base, len >= 1, tiles ascending and contiguous.
struct P3dRegTile { long long off; int len; float c; };
enum { UPD_NONE = -1, UPD_ADAM = 0, UPD_MOMENTUM = 1, UPD_SGD = 2 };      // the update kinds: P3D_OPT_* of include/p3d_hip.h
// One launch over [p, p + n).  lr_dev non-null: the step size is read from device memory (captured step graphs), lr is ignored.
//   UPD_ADAM (tf.train.AdamOptimizer, epsilon-hat form; train.py:168): lr is the bias-corrected step size; m, v its slots.
//   UPD_MOMENTUM (tf.train.MomentumOptimizer): m is the accumulator, a = (a mom) + g, then p -= lr a, or with nesterov
//     p -= (g lr) + ((a mom) lr) on the updated a.  UPD_SGD (GradientDescentOptimizer): p -= lr g.  No contraction, no fma.
//   SGD never reads m, only Adam reads v.
// ntile > 0, the decay part: one block per tile (tiles[0].off - tile_base == 0, the tiles cover [0, n)); per element
// g' = g + c*p, written back to g where c != 0, then the update on g', or nothing more under UPD_NONE (the gradient-only mode
// of p3d_backward, the same under every optimiser).  Float32 order, no contraction: g' = fadd(g, fmul(c, p)), then the update.
// Adam's float32 arithmetic is defined once (adam_elem), for the launches with and without a decay part: on 4-groups that lie
// whole in [0, n) m = fma(b1, m, (1-b1) g'), v = fma(b2, v, ((1-b2) g') g'); on a partial last group m = (b1 m) + ((1-b1) g'),
// v = (b2 v) + (((1-b2) g') g'); p -= (lr m) / (sqrt(v) + eps).  So a tile with c = 0 gives adam_kernel's bits.
// part[k] = 0.5 * c * (sum of p^2 over tile k, in double; fixed order); with nfold > 0 the last block folds
// fold_part[0 .. nfold) in index order into *term (the whole table's term, whichever ranges wrote it earlier on the stream;
// *counter zero at launch).
// Refused (hipErrorInvalidValue): Adam and every decay form unless each pointer the kernel uses is 16-byte aligned (they move
// four elements at a time); Momentum / SGD without decay unless p, g, m are float-aligned at the same place in a 16-byte line
// (the elements before the first 16-byte boundary go one by one); UPD_NONE without a decay part.
struct OptArgs {
    int update = UPD_ADAM;
    float* p = nullptr; float* g = nullptr; float* m = nullptr; float* v = nullptr;
    long n = 0;
    float lr = 0.f; const float* lr_dev = nullptr;
    float b1 = 0.f, b2 = 0.f, eps = 0.f;             // Adam
    float momentum = 0.f; int nesterov = 0;          // Momentum
    const P3dRegTile* tiles = nullptr; int ntile = 0; long long tile_base = 0;      // the decay part (ntile == 0: none)
    double* part = nullptr; const double* fold_part = nullptr; int nfold = 0; unsigned* counter = nullptr; double* term = nullptr;
    const float* gscale = nullptr;      // clipping: the *_scaled_kernel forms (below); null: the kernels above
    long long n4 = 0; int head = 0;     // the dense pass's float4 groups and leading single elements: p3d_opt_step's, not the caller's
};
// Every optimiser kernel takes the struct by value (p3d_opt_step's copy, n4 and head filled in).
// gscale non-null (p3d_set_grad_clip): a device float s, read once per block; the update runs on g'' = fmul(g', s) wherever it
// uses g' above, rounded once and not fused into the update (g' = g without a decay part).  g is still written back as g', never
// as g''.  fmul(g', 1.0f) == g', so s = 1 gives the unscaled kernels' bits.  Refused under UPD_NONE.
// decayed_elems: the elements of [p, p + n) whose tile has c != 0 (they cost 4 operations and the gradient written back)
LaunchDesc p3d_opt_desc(const OptArgs& a, double decayed_elems);
hipError_t p3d_opt_step(const OptArgs& a, hipStream_t s);
// ---- global gradient norm (p3d_set_grad_clip): grad_sumsq_kernel ---------------------------------------------------------------
// A chunk table (P3dRegTile: off relative to tile_base, len >= 1, ascending, not overlapping; elements between chunks -- slot
// padding -- belong to no chunk and are never read) cuts the gradients into pieces of one coefficient c each.  One launch sums
// chunks [k0, k1): part[k] = sum over chunk k of (double)g' * (double)g', g' = fadd(g, fmul(c, p)) in float32 without contraction
// where c != 0 (decay_body's g'), g' = g where c == 0 (p is not read).  Each square is exact in double; the sum runs in a fixed
// order that depends on the chunk's address alone.  nfold > 0 (the table's length; this launch is the last one on the stream,
// *counter zero at launch): the last block to arrive folds part[0 .. nfold) in a fixed order and writes
//   res[0] = sumsq, res[1] = norm = sqrt(sumsq) (double), and the float at res + 2:
//   scale = NaN where norm is NaN or inf; 1.0f where clip_norm is +inf; else (float)(clip_norm / max(norm, clip_norm)), both
//   in double -- exactly 1.0f whenever norm <= clip_norm.
// The three are the same bits however the table is cut into launches and whatever the grid (max_blocks; 0: the default cap).
constexpr int P3D_SUMSQ_MAX_BLOCKS = 2048;
struct SumsqArgs {
    const float* g = nullptr; const float* p = nullptr;      // p may be null when every c is 0
    const P3dRegTile* tiles = nullptr; long long tile_base = 0;
    int k0 = 0, k1 = 0;
    double* part = nullptr;      // the whole table's partials
    int nfold = 0; unsigned* counter = nullptr; double* res = nullptr;
    float clip_norm = 0.f;
    int max_blocks = 0;
};
LaunchDesc p3d_grad_sumsq_desc(const SumsqArgs& a, double elems, double decayed_elems);
hipError_t p3d_grad_sumsq(const SumsqArgs& a, hipStream_t s);
// ---- exponential moving average of the weights (p3d_set_ema): ema_kernel -------------------------------------------------------
// One launch over [s, s + n): s = fsub(s, fmul(fsub(s, p), om)) in float32, no contraction, the same on every element (TF's
// assign_moving_average with om = 1 - decay).  om_dev non-null: om is read from device memory (a captured step with warm-up, where
// it changes every step), om is ignored.  12 bytes and 3 operations per element.
// Refused (hipErrorInvalidValue): s and p not float-aligned at the same place in a 16-byte line, n < 1.
struct EmaArgs {
    float* s = nullptr; const float* p = nullptr;
    long n = 0;
    float om = 0.f; const float* om_dev = nullptr;
    long long n4 = 0; int head = 0;     // the dense pass's float4 groups and leading single elements: p3d_ema_step's, not the caller's
};
LaunchDesc p3d_ema_desc(const EmaArgs& a);
hipError_t p3d_ema_step(const EmaArgs& a, hipStream_t s);
// ---- gradient accumulation over micro-batches (p3d_set_grad_accum): grad_accum_kernel<MODE> ------------------------------------
// One launch over n elements.  GACC_STORE: acc = g, a copy of the bits; GACC_ADD: acc = fadd(acc, g); GACC_FINISH: g = fadd(acc, g)
// with acc left alone: float32, rounded once, the same on every element.  8 bytes per element for STORE, 12 for the others.
// Refused (hipErrorInvalidValue): acc and g not float-aligned at the same place in a 16-byte line, acc == g, n < 1, another mode.
enum { GACC_STORE = 0, GACC_ADD = 1, GACC_FINISH = 2 };
struct GradAccumArgs {
    float* acc = nullptr; float* g = nullptr;      // STORE / ADD write acc and read g; FINISH writes g and reads acc
    long n = 0;
    int mode = GACC_STORE;
    long long n4 = 0; int head = 0;     // the dense pass's float4 groups and leading single elements: p3d_grad_accum_step's, not the caller's
};
LaunchDesc p3d_grad_accum_desc(const GradAccumArgs& a);
hipError_t p3d_grad_accum_step(const GradAccumArgs& a, hipStream_t s);
// a and b exchanged bit for bit (p3d_ema_swap): both 16-byte aligned, n a multiple of 4
hipError_t p3d_ema_swap(float* a, float* b, long long n, hipStream_t s);
// per-step scalars of a captured train step: scal[0..1] = dropout seed (64 bit), scal[2] = the optimiser's step size (opt_step_size),
// scal[3] = the moving average's om under warm-up (ema_om); a null destination is skipped
hipError_t p3d_set_step_scalars(unsigned long long* seed_dst, float* lr_dst, float* om_dst, unsigned long long seed, float lr_t, float om,
                                hipStream_t s);
// ---- clip augmentation of the staged inputs (augment.hip; p3d_set_augment) -----------------------------------------------------
// One row of decisions per clip, applied alike to x [B,T,H,W,3], y [B,T,H,W] and the fixation bytes [B,T,H,W], out of place:
//   1 the window [y0, y0 + ch) x [x0, x0 + cw) of every frame resized back to H x W: x (each channel on its own) and y by the
//     float32 cv2.INTER_LINEAR law of resize_f32_kernel (its coordinates, float32 weights, no contraction); a fixation cell (h, w)
//     becomes 255 if the window's byte at the one (r, c) with (r - y0) * H / ch == h and (c - x0) * W / cw == w is >= 128, else 0
//     (ch <= H: at most one row and one column reach a cell).  The whole frame as the window copies the bits, bytes included;
//   2 flip: w -> W - 1 - w;  3 reverse: t -> T - 1 - t;
//   4 x only: fadd(fmul(v, a), b), each rounded on its own; a == 1 and b == 0 copies the bits.
// 1-3 are one gather and every destination element is written once.  A clip whose row is all neutral is copied 16 bytes at a time
// where source and destination of the clip are 16-byte aligned, else element by element; the gathers store element by element
// (the bytes four at a time where the clip's destination is 4-byte aligned).  Stages: AUG_X, AUG_Y, and AUG_FIX when fix is given.
// Refused (hipErrorInvalidValue) before anything is launched: a row of tab_host whose window leaves the frame, B > 65535,
// H or W > 32768, a clip of more than 2^30 elements, a source that is its destination.
struct P3dAugClip { int flip, reverse, y0, x0, ch, cw; float a, b; };
enum { AUG_X = 0, AUG_Y = 1, AUG_FIX = 2 };
struct AugArgs {
    const float* x = nullptr; const float* y = nullptr; const unsigned char* fix = nullptr;      // fix null: no AUG_FIX stage
    float* x_out = nullptr; float* y_out = nullptr; unsigned char* fix_out = nullptr;
    const P3dAugClip* tab = nullptr;           // [B], device memory
    const P3dAugClip* tab_host = nullptr;      // the same rows on the host, for the checks above
    int B = 0, T = 0, H = 0, W = 0;
};
inline int p3d_augment_stages(const AugArgs& a) { return a.fix ? 3 : 2; }
LaunchDesc p3d_augment_desc(int stage, const AugArgs& a);
hipError_t p3d_augment_launch(int stage, const AugArgs& a, hipStream_t s);

// ---- resident video inference (video.hip; p3d_video_*, the contract in include/p3d_hip.h) -----------------------------------------
// A frame store [F][frame_elems] and a map store [F][hw] with a contribution count per frame.  Four launches, each described once
// for the handle and for the hooks.  Every table reaches its kernel in device memory; the launcher checks the same rows on the
// host first (a row that leaves a buffer: hipErrorInvalidValue, nothing launched), because the kernels trust them.
//   gather   clip b of x [B][T][frame_elems] = frames starts[b] .. starts[b] + T - 1 of the store, a copy of the bits (the caller
//            pads starts to B rows with its last window).
//   scatter  one table row per destination frame, ascending by frame: `before` = the frame's count before the call and its
//            contributors src[first .. first + n), each the index k * T + t of a map of pred [maps][hw] (element stride ld),
//            ascending in k.  VIDEO_NEWEST (rows only for frames with before == 0): map = the first contributor's bits, count = 1.
//            VIDEO_MEAN: sum = before == 0 ? the first contributor's bits : the stored sum, then fadd of the others in order;
//            count = before + n.  Frames without a row keep their bits.
//   mean     out[i][hw] = __fdiv_rn(sum[i], (float)count[i]) for n frames; count 1 copies the bits.  sum != out.
enum { VIDEO_NEWEST = 0, VIDEO_MEAN = 1 };
struct P3dVideoDst { int frame, before, first, n; };
struct VideoGatherArgs {
    const float* store = nullptr; float* x = nullptr;
    const int* starts = nullptr; const int* starts_host = nullptr;      // [B], device memory / the same rows on the host
    int B = 0, T = 0, F = 0; long long frame_elems = 0;
};
struct VideoScatterArgs {
    int mode = VIDEO_NEWEST;
    const float* pred = nullptr; int ld = 1, maps = 0; long long hw = 0;
    float* store = nullptr; int32_t* count = nullptr; int F = 0;
    const P3dVideoDst* dst = nullptr; const int* src = nullptr;           // device memory
    const P3dVideoDst* dst_host = nullptr; const int* src_host = nullptr; // the same rows on the host
    int ndst = 0, nsrc = 0;
};
struct VideoMeanArgs { const float* sum = nullptr; const int32_t* count = nullptr; float* out = nullptr; int n = 0; long long hw = 0; };
LaunchDesc p3d_video_gather_desc(const VideoGatherArgs& a);
hipError_t p3d_video_gather(const VideoGatherArgs& a, hipStream_t s);
//   gather_slots  (p3d_video_predict_shots) slot i of x [B * T][frame_elems] = frame frames[i] of the store, a copy of the bits: a
//            window that reflects inside its shot is not one run of the store, so every slot names its frame.  frames [B * T] in
//            device memory, the same rows on the host; a row outside [0, F) or B * T > 65535: hipErrorInvalidValue, nothing launched.
struct VideoGatherSlotsArgs {
    const float* store = nullptr; float* x = nullptr;
    const int* frames = nullptr; const int* frames_host = nullptr;      // [B * T], device memory / the same rows on the host
    int B = 0, T = 0, F = 0; long long frame_elems = 0;
};
LaunchDesc p3d_video_gather_slots_desc(const VideoGatherSlotsArgs& a);
hipError_t p3d_video_gather_slots(const VideoGatherSlotsArgs& a, hipStream_t s);
LaunchDesc p3d_video_scatter_desc(const VideoScatterArgs& a);
hipError_t p3d_video_scatter(const VideoScatterArgs& a, hipStream_t s);
LaunchDesc p3d_video_mean_desc(const VideoMeanArgs& a);
hipError_t p3d_video_mean(const VideoMeanArgs& a, hipStream_t s);
// ---- resident training set (trainset.hip; p3d_trainset_*, the contract in include/p3d_hip.h) -------------------------------------
// V videos concatenated, video v's frames at base[v] = F_0 + .. + F_{v-1}: a frame store (TRAINSET_U8: [sum F][hw][3] bytes in the
// decoded BGR order; TRAINSET_F32: [sum F][hw][3] normalised floats), a density store [sum F][hw] bytes and a fixation store of the
// same shape.  One launch cuts clip k = frames first[k] .. first[k] + T - 1 of every tensor the call names into x [B][T][hw][3],
// y [B][T][hw] and fix [B][T][hw] (y and / or fix null: not written):
//   x    TRAINSET_U8: x[c] = __fdiv_rn(__fsub_rn((float)bgr[2 - c], mean[c]), 255.f); TRAINSET_F32: a copy of the bits
//   y    (float)((double)byte / 255.0)
//   fix  a copy of the bytes
// first [B] reaches the kernel in device memory; the launcher checks the same rows on the host first (video_host / start_host /
// first_host against frames_host [V]: a row outside its video is hipErrorInvalidValue, nothing launched): the kernel trusts them.
enum { TRAINSET_U8 = 0, TRAINSET_F32 = 1 };
struct TrainsetGatherArgs {
    int format = TRAINSET_U8;
    const void* frames = nullptr; const unsigned char* density = nullptr; const unsigned char* fixations = nullptr;      // the stores
    float* x = nullptr; float* y = nullptr; unsigned char* fix = nullptr;
    const int* first = nullptr;                                                                  // [B], device memory
    const int* first_host = nullptr; const int* video_host = nullptr; const int* start_host = nullptr;      // the same rows on the host
    const int* frames_host = nullptr; int n_videos = 0;                                          // F_v
    int B = 0, T = 0; long long hw = 0;
    float mean[3] = {0.f, 0.f, 0.f};
};
LaunchDesc p3d_trainset_gather_desc(const TrainsetGatherArgs& a);
hipError_t p3d_trainset_gather(const TrainsetGatherArgs& a, hipStream_t s);
// ---- temporal smoothing of the maps at read-out (temporal.hip; p3d_set_video_temporal, the contract in include/p3d_hip.h) -------
// One launch: frames first .. first + n - 1 of store [F][hw], filtered along the frame axis of the whole video, -> out [n][hw]
// (not the store, which is only read).  count null: a frame's input is the stored map; else [F] in device memory and the input is
// __fdiv_rn(sum, (float)count), divided as the frame is loaded (a count of 1 keeps the bits).  The caller has checked that every
// frame the read needs has a count >= 1.
//   TEMPORAL_GAUSS  w[d] = the tap w_{r+d} of p3d_blur_taps, d = 0 .. r; the PASS law with reflect-101 at frames 0 and F - 1.
//   TEMPORAL_EMA    m_0 = v_0, m_f = fadd(fmul(alpha, m_{f-1}), fmul(fsub(1, alpha), v_f)), recomputed from frame 0.
// Refused (hipErrorInvalidValue, nothing launched): a range outside [0, F), r outside 1 .. min(TEMPORAL_MAX_RADIUS, F - 1), alpha
// outside [0, 1), store == out.  The plan is a function of its four arguments alone, so a test can aim at the seams: a GAUSS block
// owns pixels_per_block pixels and frames_per_block consecutive output frames, and holds lds_bytes of LDS (at most 64 KB).
enum { TEMPORAL_OFF = 0, TEMPORAL_GAUSS = 1, TEMPORAL_EMA = 2 };
constexpr int TEMPORAL_MAX_RADIUS = 24;
struct VideoTemporalArgs {
    int kind = TEMPORAL_OFF;
    const float* store = nullptr; const int32_t* count = nullptr; float* out = nullptr;
    int F = 0; long long hw = 0; int first = 0, n = 0;
    int r = 0; float w[TEMPORAL_MAX_RADIUS + 1] = {};
    float alpha = 0.f;
};
struct VideoTemporalPlan { int threads = 0, pixels_per_block = 0, frames_per_block = 0, lds_bytes = 0; };
VideoTemporalPlan p3d_video_temporal_plan(int kind, int r, long long hw, int n);
LaunchDesc p3d_video_temporal_desc(const VideoTemporalArgs& a);
hipError_t p3d_video_temporal_launch(const VideoTemporalArgs& a, hipStream_t s);
// Under a shot table (starts [n_shots] ascending from 0, host): the runs (f0, f1, lo, hi) of a read of first .. first + n - 1, four
// ints each -- GAUSS: output frames f0 .. f1 - 1, at most the plan's frames_per_block of them, inside the shot lo .. hi; EMA: the
// shots from the one `first` lies in, each from its first frame to its last frame that is read.  The launch takes them in device
// memory and replaces rho by the shot's periodic reflect-101 (r <= F - 1 is not required), restarts the moving average at every lo.
std::vector<int> p3d_video_temporal_runs(int kind, int r, long long hw, int F, int first, int n, const int32_t* starts, int n_shots);
hipError_t p3d_video_temporal_shots_launch(const VideoTemporalArgs& a, const int* runs, int n_runs, hipStream_t s);

// ---- saliency metrics + frame pre-processing (metrics.hip; utils/metrics.py:25-287, dataflow.py:187-216) ------
hipError_t p3d_metric_cc(const float* a, const float* b, int n_maps, int n_pix, double* out, hipStream_t s);
hipError_t p3d_metric_sim(const float* a, const float* b, int n_maps, int n_pix, double* out, hipStream_t s);
hipError_t p3d_metric_nss(const float* sal, const float* fix, int n_maps, int n_pix, double* out, hipStream_t s);
int p3d_metric_auc_pad(int n_pix);      // scratch per map: pad floats (thresholds) + pad + 1 ints (counters)
hipError_t p3d_metric_auc_judd(const float* sal, const float* fix, const float* jitter, int n_maps, int n_pix, float* thr_scratch,
                               int* cnt_scratch, double* out, hipStream_t s);
hipError_t p3d_metric_fix_index(const float* fix, int n_pix, int* idx, int* count, hipStream_t s);
hipError_t p3d_metric_auc_borji(const float* sal, const float* fix, const int* rand_idx, int n_pix, int n_fix, int n_rep, double step,
                                const int* fix_idx, double* out_per_rep, hipStream_t s);
hipError_t p3d_mapf_frames(const unsigned char* bgr, int n_frames, int H0, int W0, float* dst, int H, int W, const float mean_rgb[3],
                           hipStream_t s);
hipError_t p3d_mapf_density(const unsigned char* grey, int n_frames, int H0, int W0, float* dst, int H, int W, hipStream_t s);
// the byte v of the same resize (y = v / 255.): what the training set's density store keeps
hipError_t p3d_mapf_density_u8(const unsigned char* grey, int n_frames, int H0, int W0, unsigned char* dst, int H, int W, hipStream_t s);

// ---- the same metrics at ground-truth resolution, whole-GPU reductions (metrics_full.hip; test.py:160-183) ------
// cv2.INTER_LINEAR resize of float32 maps: map m's pixel (y, x) at src[m * map_stride + (y * w + x) * elem_stride]
hipError_t p3d_resize_f32(const float* src, long long map_stride, int elem_stride, int n, int h, int w, float* dst, int H, int W,
                          hipStream_t s);
// ... and gen_pred.py's 8-bit write-out: uint8(cvRound(resize_f64(float32(map * scale)))), clamped; NaN / outside int32 -> 0.
// Writes bytes off .. off + n*H*W - 1 of dst (dst 4-byte aligned); needs H * W <= INT32_MAX.
hipError_t p3d_resize_u8(const float* src, long long map_stride, int elem_stride, int n, int h, int w, float scale, unsigned char* dst,
                         long long off, int H, int W, hipStream_t s);
// saturate_cast<uchar>(double) as cv2.imwrite's conversion to CV_8U does it on x86 (the byte law of resize_u8_kernel and of
// postprocess.hip's apply pass): round half to even, clamp to [0, 255]; NaN and a rounded value outside int32 give 0.
__device__ __forceinline__ unsigned p3d_sat_u8(double v) {
    const double r = rint(v);                                  // NaN stays NaN and fails both range tests below
    if (!(r >= -2147483648.0 && r <= 2147483647.0)) return 0u;
    return r <= 0.0 ? 0u : r >= 255.0 ? 255u : (unsigned)r;
}
struct P3dFullMaps {
    const float* P = nullptr;        // [n_maps][n_pix] saliency maps (clean)
    const float* D = nullptr;        // [n_maps][n_pix] density maps as float32(v / 255.) of the uint8 resize, or null (no CC / SIM)
    const void* fix = nullptr;       // [n_maps][n_pix] fixation maps: uint8 (>= 128) if fix_u8, else float32 (> 0.5)
    int fix_u8 = 0;
    const double* jit = nullptr;     // [n_maps][n_pix] AUC_Judd's noise, added in double and rounded to float32, or null
    long long n_pix = 0;
    int n_maps = 0, nblk = 0;        // nblk = p3d_full_blocks(n_pix) blocks per map
    const int* meta = nullptr;       // [n_maps][3]: n_fix, slot offset in fixv (cnt: + map index; room for next_pow2(n_fix) (+1)), random-index offset
    double* partA = nullptr;         // [n_maps][nblk][11]
    double* partB = nullptr;         // [n_maps][nblk][8]
    double* partC = nullptr;         // [n_maps][nblk]
    unsigned* counter = nullptr;     // [n_maps] arrival counters, zero at launch (and after)
    double* stats = nullptr;         // [n_maps][P3D_FULL_STATS]
    float* fixv = nullptr;           // fixated values of the (jittered) map, sorted descending by p3d_full_rank
    int* cnt = nullptr;              // AUC-Judd counters
    double* out = nullptr;           // [n_maps][5] CC, SIM, AUC_Judd, AUC_Borji, NSS; null: the per-split AUCs only
};
struct P3dFullBorji {
    const int* idx = nullptr;        // random pixel indices [n_rand][n_rep] per map (at meta[b][2])
    int n_rand = -1;                 // -1: n_fix rows (AUC_Borji)
    const int* n_rand_map = nullptr; // [n_maps] rows of every map instead of n_rand (device memory), or null
    int n_rep = 0;
    double step = 0.1;
    double* per_rep = nullptr;       // [n_maps][n_rep]
};
constexpr int P3D_FULL_STATS = 12;            // per map: means, minima, maxima of P, D, J; the fixation count; SIM's range sums
constexpr int P3D_FULL_STAT_NFIX = 9;         // stats[b][9]: the device's count of fixated pixels (a double)
int p3d_full_blocks(long long n_pix);
hipError_t p3d_full_moments(const P3dFullMaps& a, hipStream_t s);        // stats, CC, NSS, the fixated values
hipError_t p3d_full_rank(const P3dFullMaps& a, hipStream_t s);           // thresholds sorted; SIM, AUC_Judd
hipError_t p3d_full_borji(const P3dFullMaps& a, const P3dFullBorji& r, hipStream_t s);
// KL divergence and information gain of the same maps (p3d_set_eval_extra; the law in include/p3d_hip.h), one launch after
// p3d_full_moments: it reads pass A's stats and per-block sums (partA), P, and by flag D (KL) or fix and the baseline (IG).
enum { P3D_EXTRA_KLDIV = 1, P3D_EXTRA_INFO_GAIN = 2 };
constexpr int P3D_FULL_STATS3_PARTS = 4, P3D_FULL_EXTRA_PARTS = 3;
struct P3dFullStats3 {               // min, max, sum of n_maps maps of n_pix floats -> out[n_maps][3], pass A's order and NaN rule
    const float* maps = nullptr;
    long long n_pix = 0;
    int n_maps = 0, nblk = 0;        // nblk = p3d_full_blocks(n_pix)
    double* part = nullptr;          // [n_maps][nblk][P3D_FULL_STATS3_PARTS]
    unsigned* counter = nullptr;     // [n_maps] arrival counters, zero at launch (and after)
    double* out = nullptr;
};
struct P3dFullExtra {
    int flags = 0;                   // P3D_EXTRA_*
    const float* base = nullptr;     // IG: the baseline, ONE map [n_pix] for all maps
    const double* bstat = nullptr;   // IG: its min, max, sum (p3d_full_stats3)
    const double* sstat = nullptr;   // op level: [n_maps][3] of P by p3d_full_stats3 instead of pass A's; D is then read as it is
    const double* ystat = nullptr;   // op level with KL: [n_maps][3] of D
    double* part = nullptr;          // [n_maps][nblk][P3D_FULL_EXTRA_PARTS]
    double* out = nullptr;           // [n_maps][2]: KL, IG; NaN for a metric that is off
};
hipError_t p3d_full_stats3(const P3dFullStats3& q, hipStream_t s);
hipError_t p3d_full_extra(const P3dFullMaps& a, const P3dFullExtra& e, hipStream_t s);      // uses a.counter like the passes

// ---- smoothing and normalisation of output maps (postprocess.hip; p3d_set_postprocess, the contract in include/p3d_hip.h) -----
// One launch sequence on n maps of H x W floats, every stage optional:
//   POST_RESIZE  src given: resize_f32_kernel's float32 cv2.INTER_LINEAR law, src [n] maps of h x w -> maps;
//   POST_BLUR_H  r > 0: the horizontal pass, maps -> tmp;      POST_BLUR_V  r > 0: the vertical pass, tmp -> maps;
//   POST_PRIOR   prior given: every map multiplied by or mixed with one prior map of H x W floats, in place (prior.hip);
//   POST_MATCH   match given: histogram matching of every map, in place (hist_match.hip: p3d_hist_chain_launch on *match);
//   POST_MINMAX  norm != 0: float32 min and max of every map -> mnmx[n][2], partials folded by the last arriving block;
//   POST_APPLY   norm != 0 or u8 given: v' by `norm` stored back to maps, and sat_u8((double)fmul(v', scale)) to byte u8_off + i of
//                u8 when given (u8 4-byte aligned, u8_off arbitrary: whole words where aligned, as resize_u8_kernel).
// taps: the 2r + 1 weights in device memory (p3d_post_taps makes them on the host).  No contraction; each output element is
// computed by one lane in the header's order, whatever the tiling.  Refused (hipErrorInvalidValue) before anything is launched:
// r outside [0, P3D_POST_MAX_RADIUS] or above min(H, W) - 1, H * W above INT32_MAX, n above 65535, a missing buffer.
constexpr int P3D_POST_MAX_RADIUS = 255;
constexpr int P3D_POST_CHUNK = 16;            // maps per launch sequence of the chunked callers (scratch: 2 * 16 maps)
enum { POST_RESIZE = 0, POST_BLUR_H = 1, POST_BLUR_V = 2, POST_PRIOR = 3, POST_MATCH = 4, POST_MINMAX = 5, POST_APPLY = 6, POST_STAGES = 7 };
struct HistChain;
struct PostArgs {
    const float* src = nullptr; long long map_stride = 0; int elem_stride = 1, h = 0, w = 0;      // src null: no POST_RESIZE
    int n = 0, H = 0, W = 0;
    float* maps = nullptr;                    // [n][H][W]
    float* tmp = nullptr;                     // [n][H][W], r > 0
    const float* taps = nullptr;              // [2r + 1], r > 0
    int r = 0, norm = 0;                      // norm: P3D_NORM_*
    float* part = nullptr;                    // [n][nblk][2], norm != 0
    float* mnmx = nullptr;                    // [n][2], norm != 0
    unsigned* counter = nullptr;              // [n] arrival counters, zero at launch (and after), norm != 0
    int nblk = 0;                             // p3d_post_blocks(H * W)
    unsigned char* u8 = nullptr; long long u8_off = 0; float scale = 0.f;
    const HistChain* match = nullptr;         // POST_MATCH: its source is these n maps, remapped in place
    const float* prior = nullptr; int prior_mode = 0; float prior_a = 0.f, prior_b = 0.f;      // POST_PRIOR: PriorApplyArgs' map, mode, a, b
};
// the vertical pass's strip for radius r: cols columns x rows output rows per block, (rows + 2r) x cols floats + r + 1 taps of LDS
struct PostStrip { int cols, rows, lds_bytes; };
PostStrip p3d_post_strip(int r);              // host only; lds_bytes <= 65536 for every r in [0, P3D_POST_MAX_RADIUS]
int p3d_post_blocks(long long n_pix);
bool p3d_post_has(int stage, const PostArgs& a);
LaunchDesc p3d_post_desc(int stage, const PostArgs& a);
hipError_t p3d_post_launch(int stage, const PostArgs& a, hipStream_t s);      // a stage the arguments do not ask for: nothing, success

// ---- histogram matching of output maps (hist_match.hip; p3d_set_hist_match / p3d_match_hist, the law in include/p3d_hip.h) ----
// One launch sequence on n maps of H x W floats:
//   HIST_MINMAX  minmax_kernel of postprocess.hip -> mnmx[n][2] (this stage's own buffers: POST_MINMAX's are not touched);
//   HIST_COUNT   the tables cnt[n][nb] zeroed in stream order, then hist_count_kernel<kind>: counts (and counts[n][nb] as
//                int64 when given), centre[n][nb], cdf[n][nb]; with tcdf / tcentre (map m's target table of nt entries at
//                m * t_stride; t_stride 0: one table for all) also newv[n][nb] = interp(cdf, tcdf, tcentre);
//   HIST_REMAP   out given: out = (float)interp((double)v, centre, newv) per pixel; out may be maps.
// kind HIST_DENSITY: maps are evaluation's density maps, float32(b / 255.) of bytes b, counted as the doubles b / 255..
// Refused (hipErrorInvalidValue) before anything is launched: nb or nt outside [2, P3D_HIST_BINS_CAP], H * W above INT32_MAX, n
// above 65535, a missing buffer, a remap without a target table or of density maps.
constexpr int P3D_HIST_BINS_CAP = 1024;
enum { HIST_MINMAX = 0, HIST_COUNT = 1, HIST_REMAP = 2, HIST_STAGES = 3 };
enum { HIST_F32 = 0, HIST_DENSITY = 1 };
struct HistArgs {
    const float* maps = nullptr;              // [n][H][W]
    int kind = HIST_F32, n = 0, H = 0, W = 0, nb = 0;
    float* part = nullptr;                    // [n][nblk][2]
    float* mnmx = nullptr;                    // [n][2]
    unsigned* counter = nullptr;              // [n] arrival counters, zero at launch (and after)
    int nblk = 0;                             // p3d_post_blocks(H * W)
    int* cnt = nullptr;                       // [n][nb] the integer tables
    long long* counts = nullptr;              // [n][nb] or null
    double* cdf = nullptr; double* centre = nullptr;      // [n][nb]
    const double* tcdf = nullptr; const double* tcentre = nullptr; int nt = 0; long long t_stride = 0;
    double* newv = nullptr;                   // [n][nb], with a target table
    float* out = nullptr;                     // [n][H][W] or null: no HIST_REMAP
};
// match `source` against the table of `target` (has_target: built first, by HIST_MINMAX and HIST_COUNT on it) or a supplied one
struct HistChain { bool has_target = false; HistArgs target, source; };
bool p3d_hist_has(int stage, const HistArgs& a);
LaunchDesc p3d_hist_desc(int stage, const HistArgs& a);
hipError_t p3d_hist_launch(int stage, const HistArgs& a, hipStream_t s);         // a stage the arguments do not ask for: nothing, success
hipError_t p3d_hist_chain_launch(const HistChain& c, hipStream_t s);

// ---- fixation priors (prior.hip; p3d_prior_* / p3d_set_prior_stage, the law in include/p3d_hip.h) ------------------------------
// Count: n maps [n][n_pix] of bytes into count[n_pix], +1 per byte >= 128 (FIXATIONS) or + the byte (BYTES), times sign.  Integer
// sums modulo 2^32: one launch on n maps leaves the words of any split into several.  A subtraction below zero stores 1 to *flag
// and does not fault.  The launcher plans the cut (p3d_prior_count_plan fills the fields below the line) and refuses
// (hipErrorInvalidValue) before anything is launched: a null or misaligned count / flag, n outside [1, P3D_PRIOR_MAPS_CAP],
// n_pix outside [1, INT32_MAX], an unknown kind, a sign that is not +1 or -1.  maps may start at any byte.
constexpr long long P3D_PRIOR_MAPS_CAP = 16000000;        // 255 * maps fits a uint32
enum { P3D_PRIOR_KIND_FIXATIONS = 0, P3D_PRIOR_KIND_BYTES = 1 };
enum { P3D_PRIOR_STAGE_OFF = 0, P3D_PRIOR_STAGE_MUL = 1, P3D_PRIOR_STAGE_MIX = 2 };
struct PriorCountArgs {
    const unsigned char* maps = nullptr;      // [n][n_pix]
    long long n = 0, n_pix = 0;
    int kind = P3D_PRIOR_KIND_FIXATIONS, sign = 1;
    unsigned* count = nullptr;                // [n_pix], added to
    unsigned* flag = nullptr;                 // one word: set to 1 by a subtraction below zero, never cleared here
    // ---- the launcher's plan
    long long head = 0, words = 0, singles = 0;      // pixels ahead of the first aligned word; four-pixel word lanes; one-pixel byte lanes
    long long per_slice = 0; int slices = 1;         // maps per blockIdx.y; more than one slice: integer atomic adds
};
bool p3d_prior_count_plan(PriorCountArgs& a);
LaunchDesc p3d_prior_count_desc(const PriorCountArgs& a);       // of a planned launch
hipError_t p3d_prior_count_launch(const PriorCountArgs& a, hipStream_t s);
hipError_t p3d_prior_float(const unsigned* count, float* out, long long n_pix, hipStream_t s);      // out_i = (float)count_i, RNE
// Apply (POST_PRIOR): maps [n][n_pix] in place against prior [n_pix], b = (float)(1.0 - (double)a) formed by the caller:
//   MUL  v' = fmul(v, fadd(fmul(b, g), a));      MIX  v' = fadd(fmul(b, v), fmul(a, g)).      No contraction.
// Refused (hipErrorInvalidValue): a or b outside [0, 1], an unknown mode, n above 65535, nblk != p3d_post_blocks(n_pix).
struct PriorApplyArgs {
    float* maps = nullptr; const float* prior = nullptr;
    int n = 0, n_pix = 0, mode = P3D_PRIOR_STAGE_OFF, nblk = 0;
    float a = 0.f, b = 1.f;
};
LaunchDesc p3d_prior_apply_desc(const PriorApplyArgs& q);
hipError_t p3d_prior_apply_launch(const PriorApplyArgs& q, hipStream_t s);

// ---- fixation pool and shuffled AUC's sampling (fixpool.hip; p3d_fixpool_* / p3d_eval_shuffled_*, the law in include/p3d_hip.h) ---
// Pack: n maps [n][n_pix] of bytes -> words [n][nw], nw = ceil(n_pix / 64): bit j of word k is set exactly when byte 64k + j of the
// map is >= 128, the high bits of a map's last word are 0.  Every word has one writer and is stored whole.  maps may start at any
// byte.  Refused (hipErrorInvalidValue): a null or misaligned buffer, n outside [1, 65535], n_pix outside [1, 2^30].
constexpr int P3D_FIX_SCAN_WORDS = 256;                   // words per block of the union's scan: block seams at multiples of it
struct FixPackArgs {
    const unsigned char* maps = nullptr;      // [n][n_pix]
    long long n = 0, n_pix = 0;
    unsigned long long* words = nullptr;      // [n][nw]
};
__host__ __device__ inline long long p3d_fix_words(long long n_pix) { return (n_pix + 63) / 64; }
LaunchDesc p3d_fix_pack_desc(const FixPackArgs& a);
hipError_t p3d_fix_pack_launch(const FixPackArgs& a, hipStream_t s);
// Union: uni[b][k] = OR over m < M of pool[ids[b][m]][k]; prefix[b][k] = the set bits of uni[b] in the words before k of k's scan
// block (P3D_FIX_SCAN_WORDS words); bsum[b][j] = the set bits in the scan blocks before j; n_other[b] = all of them.  uint32
// integer sums.  The last arriving block of a map (det_reduce.h's ticket on counter[b], zero at launch and after) scans the block
// sums.  Refused: a missing buffer, B outside [1, 65535], M outside [1, 64], nsb != ceil(nw / P3D_FIX_SCAN_WORDS).  The ids are
// the caller's to check.
struct FixUnionArgs {
    const unsigned long long* pool = nullptr; // [capacity][nw]
    long long nw = 0;
    const int* ids = nullptr;                 // [B][M] pool slots (device memory)
    int B = 0, M = 0, nsb = 0;
    unsigned long long* uni = nullptr;        // [B][nw]
    unsigned* prefix = nullptr;               // [B][nw]
    unsigned* bsum = nullptr;                 // [B][nsb]
    unsigned* n_other = nullptr;              // [B]
    unsigned* counter = nullptr;              // [B]
};
inline int p3d_fix_scan_blocks(long long nw) { return (int)((nw + P3D_FIX_SCAN_WORDS - 1) / P3D_FIX_SCAN_WORDS); }
LaunchDesc p3d_fix_union_desc(const FixUnionArgs& a);
hipError_t p3d_fix_union_launch(const FixUnionArgs& a, hipStream_t s);
// Select: map b has n_rows[b] * n_rep ranks at ranks[meta[b][2] ..), row-major [n_rows][n_rep] (P3dFullMaps' meta: the random-index
// offset); out[i] = the pixel index of the ranks[i]-th set bit of uni[b], np.nonzero(other)[0][rank].  A rank outside
// [0, n_other[b]) is the caller's to refuse; the kernel writes 0 for it.
struct FixSelectArgs {
    const unsigned long long* uni = nullptr; const unsigned* prefix = nullptr; const unsigned* bsum = nullptr; const unsigned* n_other = nullptr;
    long long nw = 0;
    int B = 0, nsb = 0, n_rep = 0, max_rows = 0;          // max_rows: the largest n_rows (sizes the grid)
    const int* meta = nullptr;                // [B][3]
    const int* n_rows = nullptr;              // [B] (device memory)
    const int* ranks = nullptr;
    int* out = nullptr;
};
LaunchDesc p3d_fix_select_desc(const FixSelectArgs& a);
hipError_t p3d_fix_select_launch(const FixSelectArgs& a, hipStream_t s);

// ---- scoring 8-bit maps against 8-bit ground truth (score_u8.hip; p3d_video_score / p3d_score_maps_u8, the law in include/p3d_hip.h) ----
// One launch sequence on n maps of n_pix bytes, 1 <= n_pix <= 2^23, sal / den / fix [n][n_pix] (fix may be null: nothing is fixated;
// den may be null when none of CC, SIM and KL is selected: pass A then counts neither hd nor the products, and reads no density):
//   SCORE_COUNT  tab[n][P3D_SCORE_TAB_WORDS] zeroed in stream order, then score_count_kernel: hs[256], hf[256], hd[256] and the
//                64-bit sum of s * d of every map; the last arriving block of a map (counter[m]) writes out[m][0 .. 5) -- CC, NaN,
//                AUC_Judd, NaN, NSS, an unselected column NaN -- and, with SIM or KL selected, lut[m][4][256]: us, ud, ps, pd;
//   SCORE_TERMS  with SIM or KL selected only: score_terms_kernel, block partials in part[n][nblk][2], the last arriving block of
//                a map (counter[n + m]) folds them in block order into out[m][1] and out[m][3].
// Refused (hipErrorInvalidValue): a missing buffer, n outside [1, 65535], n_pix outside the range, flags outside the five bits, an
// unknown ties law, JUDD or NSS without fix, nblk / chunk other than p3d_score_plan's.
constexpr int P3D_SCORE_TAB_WORDS = 770;                  // 3 * 256 counters, then the sum of products as two words (8-byte aligned)
constexpr int P3D_SCORE_MAX_PIXELS = 1 << 23;             // 65025 * 2^46 < 2^63: every integer of FINALISE fits a signed 64-bit word
constexpr int P3D_SCORE_ALL = 31;
enum { SCORE_COUNT = 0, SCORE_TERMS = 1, SCORE_STAGES = 2 };
struct ScoreArgs {
    const unsigned char* sal = nullptr; const unsigned char* den = nullptr; const unsigned char* fix = nullptr;
    int n = 0, n_pix = 0, flags = 0, ties = 0;
    int nblk = 0, chunk = 0;                  // p3d_score_plan(n_pix)
    unsigned* tab = nullptr;                  // [n][P3D_SCORE_TAB_WORDS]
    double* lut = nullptr;                    // [n][4][256]
    double* part = nullptr;                   // [n][nblk][2]
    unsigned* counter = nullptr;              // [2 n]
    double* out = nullptr;                    // [n][5]
};
// blocks per map (one per 32768 pixels, at most 256) and pixels per block, a multiple of 16 so that every block of a map starts as
// far past a 16-byte boundary as the map does
struct ScorePlan { int nblk = 0, chunk = 0; };
ScorePlan p3d_score_plan(long long n_pix);
// How a block cuts its len pixels: `head` single pixels up to the first 16-byte boundary, `words` whole 16-byte words, the rest
// single.  Sources that are not aligned alike: every pixel single.
struct ScoreCut { int head, words; };
__host__ __device__ inline ScoreCut p3d_score_cut(uintptr_t as, uintptr_t ad, uintptr_t ax, int len) {
    if (((as ^ ad) & 15) || ((as ^ ax) & 15)) return {len, 0};
    const int head = (int)((16 - (as & 15)) & 15);
    if (head >= len) return {len, 0};
    return {head, (len - head) >> 4};
}
// the most products s * d any lane of pass A adds, for n maps whose sources start off_s / off_d / off_x bytes past a 16-byte boundary
long long p3d_score_lane_products(long long n_pix, int n, unsigned off_s, unsigned off_d, unsigned off_x);
bool p3d_score_has(int stage, const ScoreArgs& a);
LaunchDesc p3d_score_desc(int stage, const ScoreArgs& a);
hipError_t p3d_score_launch(int stage, const ScoreArgs& a, hipStream_t s);      // a stage the arguments do not ask for: nothing, success

// ---- AUC-Borji and shuffled AUC of 8-bit maps (score_auc_u8.hip; p3d_score_sweep_u8 / p3d_video_score_auc, the law in
// include/p3d_hip.h, SPLIT SWEEP) ----
//   SWEEP_PREP  per map, from pass A's tables tab (SCORE_COUNT, earlier in the stream): lev[n][256], the fixation ladder
//               lad[n][kmax + 1] (lad[l] = sum of hf[v] over lev[v] >= l) and info[n][4] = {nf, lo, hi, maxfix} (-1: none);
//   SWEEP_RUN   per (split, map): map m's n_rows = meta[m][0] rows of n_rep pixel indices start at idx[meta[m][1]]; the bytes
//               sal[m][idx] are gathered and counted per level, per_rep[m][split] is the area (NaN: nf = 0 or a flat map) and,
//               where top is not null, top[m][split] the split's largest byte or maxfix.  One prep serves any number of runs.
// Refused (hipErrorInvalidValue): a missing buffer, n outside [1, 65535], n_pix outside the range, kmax other than
// p3d_sweep_kmax(step) or 0, n_rep < 1, cols other than p3d_sweep_cols'.  Indices outside [0, n_pix) are the caller's to refuse.
constexpr int P3D_SWEEP_MAX_KMAX = 1024;
enum { SWEEP_PREP = 0, SWEEP_RUN = 1, SWEEP_STAGES = 2 };
struct ScoreSweepArgs {
    const unsigned char* sal = nullptr;       // [n][n_pix]
    const unsigned* tab = nullptr;            // [n][P3D_SCORE_TAB_WORDS], pass A's
    int n = 0, n_pix = 0, kmax = 0, n_rep = 0, cols = 0;
    double step = 0.0;
    int* lev = nullptr;                       // [n][256]
    unsigned* lad = nullptr;                  // [n][kmax + 1]
    int* info = nullptr;                      // [n][4]
    const int* idx = nullptr;
    const long long* meta = nullptr;          // [n][2]
    int* top = nullptr;                       // [n][n_rep], or null
    double* per_rep = nullptr;                // [n][n_rep]
};
int p3d_sweep_kmax(double step);              // (int)ceil(1 / step); 0: not positive, or more than P3D_SWEEP_MAX_KMAX thresholds
// split columns of a block: a power of two <= 32 whose histograms (kmax + 1 counters a split) fit 48 KB, no wider than n_rep needs
int p3d_sweep_cols(int kmax, int n_rep);
LaunchDesc p3d_sweep_desc(int stage, const ScoreSweepArgs& a);
hipError_t p3d_sweep_launch(int stage, const ScoreSweepArgs& a, hipStream_t s);

// ---- overlays of 8-bit maps on their frames (render.hip; p3d_video_render / p3d_render_u8, the law in include/p3d_hip.h) ----
// One launch on n maps of H x W bytes: sal [n][H][W], frames [n][H][W][3] (null: the heat map), table [256] in device memory,
// out [n][H][W][3].  level > 0: the contour of {s >= level}, thick pixels wide, in contour_bgr.  Without a contour the blocks are
// flat runs of RENDER_CHUNK pixels; with one they are tiles of RENDER_TILE_ROWS x RENDER_TILE_COLS pixels.
// Refused (hipErrorInvalidValue): a missing buffer, n outside [1, 65535], H * W outside [1, 2^28], level outside [0, 255], with a
// contour thick outside [1, 4], a plan other than p3d_render_plan's.
constexpr int P3D_RENDER_MAX_PIXELS = 1 << 28;            // 3 H W fits int32 inside a map
constexpr int P3D_RENDER_MAX_THICKNESS = 4;
constexpr int RENDER_CHUNK = 8192;                        // a multiple of 16: every block of a map starts as far past a boundary as the map
constexpr int RENDER_TILE_ROWS = 16, RENDER_TILE_COLS = 256;
constexpr int RENDER_GRID_X = 65536;                      // blocks of a map in the grid's x; a map of more folds the rest into z (<= 2^24 / 2^16)
struct RenderPlan { int rows = 0, cols = 0, chunk = 0; long long blocks = 0; };      // rows = cols = 0: flat runs of chunk pixels
RenderPlan p3d_render_plan(int H, int W, int thick /* 0: no contour */);
struct RenderArgs {
    const unsigned char* sal = nullptr; const unsigned char* frames = nullptr; unsigned char* out = nullptr;
    const unsigned* table = nullptr;          // [256]: b | g << 8 | r << 16 | o << 24
    int n = 0, H = 0, W = 0;
    int level = 0, thick = 0;
    unsigned char contour_bgr[4] = {0, 0, 0, 0};
    int rows = 0, cols = 0, chunk = 0; long long blocks = 0;      // p3d_render_plan(H, W, level > 0 ? thick : 0)
};
// How a run of len pixels is cut: `head` single pixels up to the first 16-byte boundary of s, `words` groups of 16 pixels, the
// rest single.  Frame and out bytes of pixel p start 3 p past their base, so the three are aligned alike exactly when the frame
// and out addresses equal 3 times the s address modulo 16; otherwise every pixel is single.
struct RenderCut { int head, words; };
__host__ __device__ inline RenderCut p3d_render_cut(uintptr_t as, uintptr_t af, uintptr_t ao, int len) {
    if (((af - 3 * as) & 15) || ((ao - 3 * as) & 15)) return {len, 0};
    const int head = (int)((16 - (as & 15)) & 15);
    if (head >= len) return {len, 0};
    return {head, (len - head) >> 4};
}
hipError_t p3d_render_launch(const RenderArgs& a, hipStream_t s);

// ---- reframing around 8-bit maps (reframe.hip; p3d_video_reframe / p3d_reframe_u8, the law in include/p3d_hip.h) ----
// One launch sequence on n maps of H x W bytes: sal [n][H][W], frames [n][H][W][3] (null: tracks and masses only) -> track [n][2]
// (Y, X), raw [n][2], mass [n][3] (M_best, M_smoothed, T), out [n][hc][wc][3] (null exactly when frames is); every buffer device
// memory.  sat, best and part are scratch of p3d_reframe_plan's sat_elems, best_elems and part_elems words; sat starts on a 16-byte
// boundary.  Per chunk of maps_per_chunk maps: the summed-area tables (two launches), the search, the pick; then the track, the
// masses at the track's positions (two launches) and the crop.
// Refused (hipErrorInvalidValue): a missing buffer, frames without out or out without frames, n outside [1, 65535], H * W outside
// [1, 2^23], a window outside [1, H] x [1, W], a gate or radius outside [0, 255], a plan other than p3d_reframe_plan's, starts
// without n_shots in 1 .. n or n_shots without starts (the table's values are the caller's to check: they are device memory).
constexpr int P3D_REFRAME_MAX_PIXELS = 1 << 23;           // 255 * 2^23 < 2^31: a mass fits one unsigned word
constexpr int P3D_REFRAME_CHUNK = 16;                     // at most this many maps' tables at a time, as P3D_POST_CHUNK
constexpr long long P3D_REFRAME_SAT_BYTES = 64LL << 20;   // and at most this many bytes of tables (never less than one map's)
constexpr int REFRAME_POSITIONS = 4096;                   // window positions a block of the search takes
constexpr int REFRAME_MASS_SLICES = 16;                   // blocks that share the rows of one window when its mass is re-summed
struct ReframePlan {
    int maps_per_chunk = 0, positions_per_block = 0, search_blocks = 0;
    long long sat_elems = 0, best_elems = 0, part_elems = 0, scratch_bytes = 0;
};
ReframePlan p3d_reframe_plan(int H, int W, int hc, int wc, int n);
struct ReframeArgs {
    const unsigned char* sal = nullptr; const unsigned char* frames = nullptr; unsigned char* out = nullptr;
    int32_t* track = nullptr; int32_t* raw = nullptr; uint32_t* mass = nullptr;
    unsigned* sat = nullptr; unsigned* best = nullptr; unsigned* part = nullptr;
    int n = 0, H = 0, W = 0, hc = 0, wc = 0, gate = 0, radius = 0;
    int maps_per_chunk = 0, search_blocks = 0;            // p3d_reframe_plan(H, W, hc, wc, n)
    const int32_t* starts = nullptr; int n_shots = 0;     // a shot table in frames of the call (device; ascending from 0), or none
};
hipError_t p3d_reframe_launch(const ReframeArgs& a, hipStream_t s);

// ---- connected regions of 8-bit maps (regions.hip; p3d_video_regions / p3d_regions_u8, the law in include/p3d_hip.h) ----
// One launch sequence on n maps of H x W bytes: sal [n][H][W] -> regions [n][K][P3D_REGIONS_NFIELDS] int32, counts [n][3] int32 and
// label maps (lab); every buffer device memory.  A root's statistics live in tables indexed by SLOT(root) = y * ceil(W / 2) + x / 2
// (two roots never share a slot: the pixels 2k and 2k + 1 of a row are neighbours), `slots` of them a map.  Scratch, for
// p3d_regions_plan's maps_per_chunk maps at a time: parent [maps][H W] words (a foreground pixel's root; the background's entries are
// never touched), tab32 [maps][7][slots] (area, mass, y0, x0, y1, x1, peak key), tab64 [maps][2][slots] (SY, SX), rank [maps][slots]
// bytes, keys [maps][slots] (the roots in arrival order, then their selection keys), cnt [maps][2] (components, regions kept), ovl
// [maps][K][K] and state [2 + K] (link only).  lab: [n][H W] bytes when lab_full (the caller wants the label maps), else, under link,
// a ring of maps_per_chunk + 1 maps with frame f in slot (f + 1) mod that; null when neither.
// Refused (hipErrorInvalidValue): a missing buffer, n outside [1, 65535], H * W outside [1, 2^23], a gate outside [1, 255], a
// connectivity other than 4 or 8, min_area < 1, K outside [1, 64], a plan other than p3d_regions_plan's, starts without n_shots in
// 1 .. n or n_shots without starts.
constexpr int P3D_REGIONS_MAX_PIXELS = 1 << 23;               // 255 * 2^23 < 2^31: every field of a record fits int32
constexpr int P3D_REGIONS_K = 64;                             // P3D_REGIONS_MAX of the header
constexpr int P3D_REGIONS_NFIELDS = 15;                       // P3D_REGION_FIELDS of the header
constexpr int P3D_REGIONS_CHUNK = 16;                         // at most this many maps' tables at a time
constexpr long long P3D_REGIONS_SCRATCH_BYTES = 512LL << 20;  // and at most this many bytes of them (never less than one map's): 16 maps of 1080 x 960
constexpr int P3D_REGIONS_TAB32 = 7, P3D_REGIONS_TAB64 = 2;   // 32- and 64-bit statistics a slot
constexpr int REGIONS_TILE_H = 32, REGIONS_TILE_W = 64;       // the labelling's tile: a wave a row, a lane a column
struct RegionsPlan {
    int tile_h = 0, tile_w = 0, tiles_y = 0, tiles_x = 0, maps_per_chunk = 0;
    long long slots = 0, parent_elems = 0, tab32_elems = 0, tab64_elems = 0, rank_elems = 0, key_elems = 0, cnt_elems = 0,
              ovl_elems = 0, state_elems = 0, lab_elems = 0, scratch_bytes = 0;
};
RegionsPlan p3d_regions_plan(int H, int W, int n, int K, int link, int lab_full);
struct RegionsArgs {
    const unsigned char* sal = nullptr; int32_t* regions = nullptr; int32_t* counts = nullptr; unsigned char* lab = nullptr;
    unsigned* parent = nullptr; unsigned* tab32 = nullptr; unsigned long long* tab64 = nullptr; unsigned char* rank = nullptr;
    unsigned long long* keys = nullptr; unsigned* cnt = nullptr; unsigned* ovl = nullptr; int32_t* state = nullptr;
    int n = 0, H = 0, W = 0, gate = 0, conn = 0, min_area = 0, K = 0, link = 0, lab_full = 0;
    int maps_per_chunk = 0, tiles_y = 0, tiles_x = 0; long long slots = 0;      // p3d_regions_plan(H, W, n, K, link, lab_full)
    const int32_t* starts = nullptr; int n_shots = 0;        // a shot table in frames of the call (device; ascending from 0), or none
};
hipError_t p3d_regions_launch(const RegionsArgs& a, hipStream_t s);

// ---- block importance and QP offsets of 8-bit maps (qpmap.hip; p3d_video_qpmap / p3d_qpmap_u8, the law in include/p3d_hip.h) ----
// One launch sequence on n maps of H x W bytes: sal [n][H][W] -> qp [n][Hb][Wb] int32 (q2), levels [n][Hb][Wb] bytes (L', or null) and
// stats [n][4] int32 (or null), Hb = ceil(H / block), Wb = ceil(W / block); every buffer device memory, law [256] and starts too.
// Scratch: lev0 [maps_per_chunk][Hb][Wb] bytes, the levels before DILATE of p3d_qpmap_plan's maps_per_chunk maps at a time.  qp holds
// q0, then q1, then q2, each in place of the one before.
// Refused (hipErrorInvalidValue): a missing buffer, n outside [1, 65535], H * W outside [1, 2^23], a configuration outside the header's
// ranges, a plan other than p3d_qpmap_plan's, starts without n_shots in 1 .. n or n_shots without starts.  The law's entries are the
// caller's to check: they live on the device.
constexpr int P3D_QPMAP_MAX_PIXELS = 1 << 23;                 // 127 * 2^23 < 2^31: an area-weighted sum of offsets fits int32
constexpr int P3D_QPMAP_CHUNK = 64;                           // at most this many maps' first levels at a time
constexpr int QPMAP_TILE_WORDS = 256;                         // the reduction's tile: `block` rows of this many 16-byte words of a row
struct QpmapPlan {
    int strip_rows = 0, tile_cols = 0, tiles_x = 0, Hb = 0, Wb = 0, blocks_per_map = 0, maps_per_chunk = 0;
    long long lev0_elems = 0, scratch_bytes = 0;
};
QpmapPlan p3d_qpmap_plan(int H, int W, int block, int n);
struct QpmapArgs {
    const unsigned char* sal = nullptr; const int32_t* law = nullptr; int32_t* qp = nullptr; unsigned char* levels = nullptr;
    int32_t* stats = nullptr; unsigned char* lev0 = nullptr;
    int n = 0, H = 0, W = 0, block = 0, peak_weight = 0, dilate = 0, fall = 0, rise = 0, balance = 0, target = 0, lo = 0, hi = 0;
    int maps_per_chunk = 0, Hb = 0, Wb = 0, tiles_x = 0;      // p3d_qpmap_plan(H, W, block, n)
    const int32_t* starts = nullptr; int n_shots = 0;        // a shot table in frames of the call (device; ascending from 0), or none
};
hipError_t p3d_qpmap_launch(const QpmapArgs& a, hipStream_t s);

// ---- frames low-pass filtered away from their saliency (prefilter.hip; p3d_video_prefilter / p3d_prefilter_u8, the law in include/p3d_hip.h) ----
// One launch sequence on n frames of H x W pixels: frames [n][H][W][3] and the strength grid [n][Hb][Wb] int32 that p3d_qpmap_launch
// left (0 .. 64) -> out [n][H][W][3]; every buffer device memory.  Scratch: tmp[0] (passes >= 2) and tmp[1] (passes = 3), each
// p3d_prefilter_plan's tmp_bytes, the intermediate passes of frames_per_chunk frames at a time.
// Refused (hipErrorInvalidValue): a missing buffer, n outside [1, 65535], H * W outside [1, 2^23], a block, radius or pass count
// outside the header's ranges, a plan other than p3d_prefilter_plan's.  The grid's entries are the caller's to keep in 0 .. 64.
constexpr int P3D_PREFILTER_MAX_PIXELS = 1 << 23;             // the grid is the QP maps'
constexpr int P3D_PREFILTER_MAX_RADIUS = 16, P3D_PREFILTER_MAX_PASSES = 3;
constexpr int PREFILTER_TILE_ROWS = 32, PREFILTER_TILE_COLS = 64;      // pixels of a block's tile; both above the largest radius
constexpr long long P3D_PREFILTER_CHUNK_BYTES = 1LL << 26;    // an intermediate pass holds at most this many bytes (and at least a frame)
struct PrefilterPlan {
    int tile_rows = 0, tile_cols = 0, halo = 0, fused = 0, tiles_x = 0, tiles_y = 0, Hb = 0, Wb = 0, frames_per_chunk = 0;
    long long blocks_per_frame = 0, tmp_bytes = 0, scratch_bytes = 0;
    unsigned mul = 0; int shift = 0;                          // floor(x / (2 (2 R + 1)^2)) = (x * mul) >> shift for 0 <= x < 2^20
};
PrefilterPlan p3d_prefilter_plan(int H, int W, int block, int radius, int passes, int n);
struct PrefilterArgs {
    const unsigned char* frames = nullptr; unsigned char* out = nullptr; const int32_t* grid = nullptr;
    unsigned char* tmp[2] = {nullptr, nullptr};
    int n = 0, H = 0, W = 0, block = 0, radius = 0, passes = 0;
    int Hb = 0, Wb = 0, tiles_x = 0, tiles_y = 0, frames_per_chunk = 0; unsigned mul = 0; int shift = 0;      // p3d_prefilter_plan(H, W, block, radius, passes, n)
};
hipError_t p3d_prefilter_launch(const PrefilterArgs& a, hipStream_t s);

// ---- distortion of frames under their 8-bit maps (distortion.hip; p3d_video_distortion / p3d_distortion_u8, the law in include/p3d_hip.h) ----
// One launch sequence on n frames of H x W pixels: sal [n][H][W], ref and test [n][H][W][3] and the weight law wlaw [256] (0 .. 255)
// -> table [n][P3D_DISTORTION_RECORD] int64 and, with block != 0 and block_sse set, block_sse [n][Hb][Wb] int64; every buffer device
// memory.  The launches zero both outputs themselves and add to them with 64-bit integer atomics: no scratch, and no order can show.
// Refused (hipErrorInvalidValue): a missing buffer, n outside [1, 65535], H * W outside [1, 2^23], a block or gate outside the
// header's ranges, a block map with block = 0, a plan other than p3d_distortion_plan's.  The law's entries are the caller's to keep
// in 0 .. 255: the 32-bit partial sums are proven for those.
constexpr int P3D_DISTORTION_MAX_PIXELS = 1 << 23;
constexpr int DISTORTION_TILE_ROWS = 64, DISTORTION_TILE_COLS = 128;      // pixels of a block's tile in the sums' launch
constexpr int DISTORTION_SSIM_ROWS = 32, DISTORTION_SSIM_COLS = 64;       // pixels of a block's tile in the SSIM launch: 8 x 16 windows
struct DistortionPlan {
    int tile_rows = 0, tile_cols = 0, tiles_x = 0, tiles_y = 0, Hb = 0, Wb = 0;
    int win_rows = 0, win_cols = 0, ssim_tiles_x = 0, ssim_tiles_y = 0;      // SSIM windows a frame, and the tiles that hold their corners
    long long blocks_per_frame = 0, scratch_bytes = 0;
};
DistortionPlan p3d_distortion_plan(int H, int W, int block, int n);
struct DistortionArgs {
    const unsigned char* sal = nullptr; const unsigned char* ref = nullptr; const unsigned char* test = nullptr;
    const int32_t* wlaw = nullptr; long long* table = nullptr; long long* block_sse = nullptr;
    int n = 0, H = 0, W = 0, block = 0, gate = 0;
    int Hb = 0, Wb = 0, tiles_x = 0, tiles_y = 0, win_rows = 0, win_cols = 0, ssim_tiles_x = 0, ssim_tiles_y = 0;      // p3d_distortion_plan(H, W, block, n)
};
hipError_t p3d_distortion_launch(const DistortionArgs& a, hipStream_t s);

// ---- shot boundaries of 8-bit frames (shots.hip; p3d_shot_distances_u8 / p3d_shot_cuts, the law in include/p3d_hip.h) ----
// The cut signal of n frames [n][H][W][3] of device bytes: D [n] device words, D_0 = 0, D_f the distance of frame f's cell
// histograms from frame f - 1's.  tabs is scratch of (frames_per_chunk + 1) tables of table_words words on a 16-byte boundary: slot 0
// holds the last table of the chunk before, slots 1 .. the chunk's frames.  Per chunk: a fill of its slots, the count (grid
// (blocks_per_frame, frames)), the distances (a block a frame), and a copy of the last slot to slot 0.  ballot: 1 aggregates a wave's
// equal bins as score_u8.hip's count_bin does, 0 adds every byte on its own (the counts are the same; the time is not).
// Refused (hipErrorInvalidValue): a missing buffer, n outside [1, 65535], H * W outside [1, 2^28], a grid outside
// [1, min(4, H)] x [1, min(4, W)], a plan other than p3d_shots_plan's.
constexpr long long P3D_SHOTS_MAX_PIXELS = 1LL << 28;     // D_f <= 6 P < 2^32
constexpr int P3D_SHOTS_CHUNK = 64;                       // at most this many frames' tables at a time
constexpr int SHOTS_BLOCK_BYTES = 64 << 10;               // a block of the count takes whole rows of at most about this many bytes together
constexpr int P3D_SHOTS_BALLOT = 0;                       // what the entry points count with: plain adds (ballot took 1.4 - 1.8 times as long)
struct ShotsPlan {
    int rows_per_block = 0, blocks_per_frame = 0, frames_per_chunk = 0, table_words = 0;
    long long scratch_bytes = 0;
};
ShotsPlan p3d_shots_plan(int H, int W, int gy, int gx, int n);
struct ShotsArgs {
    const unsigned char* frames = nullptr; uint32_t* D = nullptr; unsigned* tabs = nullptr;
    int n = 0, H = 0, W = 0, gy = 0, gx = 0, ballot = 0;
    int rows_per_block = 0, blocks_per_frame = 0, frames_per_chunk = 0;      // p3d_shots_plan(H, W, gy, gx, n)
};
hipError_t p3d_shots_launch(const ShotsArgs& a, hipStream_t s);
// The cut decision on D [F] device words (one block): cand is scratch of F words; starts [cap] receives the first min(cap, n_shots)
// shot starts, n_shots [1] their number.  P = H * W of the frames D came from.
struct ShotCutArgs {
    const uint32_t* D = nullptr; unsigned* cand = nullptr; int32_t* starts = nullptr; int32_t* n_shots = nullptr;
    int F = 0, cap = 0; long long P = 0;
    int threshold_permille = 0, window = 0, ratio_q8 = 0, min_length = 0;
};
hipError_t p3d_shot_cuts_launch(const ShotCutArgs& a, hipStream_t s);
// The three signals of "Gradual transitions" (p3d_shot_signals_u8): cut.D as above, E [n] the distance of frame f's histograms
// from frame f - lag's (0 for f < lag; lag 0: all 0) and v [n] the spread of the frame's bins.  cut carries the frames, the grid and
// the count's plan, which is p3d_shots_plan's; cut.tabs is scratch of p3d_transitions_plan's `tables` tables: the first carry =
// max(lag, 1) slots hold the last tables of the chunk before, frame c of the chunk is slot carry + c.  Per chunk: a fill of its
// slots, shots_count unchanged, one block a frame for D, E and v together, and a copy of the chunk's last carry tables to the front.
// Refused (hipErrorInvalidValue): what p3d_shots_launch refuses, a missing E or v, a lag other than 0 or 2 .. P3D_SHOTS_MAX_LAG.
constexpr int P3D_SHOTS_MAX_LAG = 64;                     // a chunk's carry comes from one chunk: P3D_SHOTS_MAX_LAG <= P3D_SHOTS_CHUNK
struct TransitionsPlan {
    int tables = 0;                                       // min(n, P3D_SHOTS_CHUNK) + max(lag, 1)
    long long scratch_bytes = 0;                          // tables * gy * gx * 192 * 4
};
TransitionsPlan p3d_transitions_plan(int gy, int gx, int n, int lag);
struct ShotSignalsArgs {
    ShotsArgs cut;
    uint32_t* E = nullptr; long long* v = nullptr;
    int lag = 0;
};
hipError_t p3d_shot_signals_launch(const ShotSignalsArgs& a, hipStream_t s);
// The decision of "Gradual transitions" on D, E, v [F] (one block): flags and marks are scratch of F words each; starts and kinds
// [cap] receive the first min(cap, n_shots) shots, n_shots [1] their number.  cut holds D, the cut rule, F, P and cap; its cand,
// starts and n_shots are the ones used.  Refused: what p3d_shot_cuts_launch refuses, a missing buffer, a CONFIG value outside its range.
struct ShotTransitionArgs {
    ShotCutArgs cut;
    const uint32_t* E = nullptr; const long long* v = nullptr; unsigned* marks = nullptr; int32_t* kinds = nullptr;
    int lag = 0, high_permille = 0, dip_q8 = 0, mono_q8 = 0, mono_min = 0;
};
hipError_t p3d_shot_transitions_launch(const ShotTransitionArgs& a, hipStream_t s);

// ---- misc ---------------------------------------------------------------------------------------
hipError_t p3d_add_inplace(float* dst, int lddst, const float* src, int ldsrc, long M, int C, hipStream_t s);
hipError_t p3d_copy_strided(float* dst, int lddst, const float* src, int ldsrc, long M, int C, hipStream_t s);
hipError_t p3d_fill_uniform(float* p, long n, float lo, float hi, unsigned long long seed, hipStream_t s);
// one block that holds stream `s` for delay_us (1 .. 2000) microseconds, bounded, and touches no memory (p3d_debug_perturb)
hipError_t p3d_delay(int delay_us, hipStream_t s);
hipError_t p3d_fill_trunc_normal(float* p, long n, float stddev, unsigned long long seed, hipStream_t s);   // N(0, stddev) within 2 stddev
hipError_t p3d_colsum(const float* dy, int ld, long M, int C, float* out, hipStream_t s);   // out += column sums
// stem re-layout (elementwise.hip): 3-channel input -> 4-channel rows with the W padding written out; packed weights
hipError_t p3d_stem_pad(const float* x, float* x4, long long rows, int W, int Wp, int pad, hipStream_t s);
hipError_t p3d_stem_pack_w(const float* w, float* w4, int taps_hw, int Co, hipStream_t s);          // [kh*kw][3][Co] -> [kh*kw][4][Co]
hipError_t p3d_stem_unpack_dw(const float* dw4, float* dw, int taps_hw, int Co, hipStream_t s);     // dw += the 3 real channels of dw4
// stem filter gradient in one pass over the output gradient (stem_wgrad.hip): [1,7,7,3,64], stride [1,2,2], even output width
struct StemWgradArgs {
    const float* x4; int Wp; int Hi;           // the padded 4-channel copy of the clip [nimg*Hi][Wp][4] (p3d_stem_pad)
    int nimg, Ho, Wo, pad_h;                   // nimg = N*D frames; SAME padding above the image
    const float* dy; int lddy;                 // output gradient [nimg*Ho*Wo][64]; fused: the gradient of the BatchNorm + ReLU OUTPUT
    int fused;                                 // 1: dy is differentiated through bn -> relu on the fly (bn_bwd_apply, mode 0)
    const float* y; int ldy;                   // fused: the conv's output (the BatchNorm's input)
    const float* scale; const float* shift; const float* mean; const float* invstd; const float* gamma;
    const float* coef; int batch;              // fused: (sum g / M, sum g*xhat / M) per channel (bn_bwd_finalize); batch = 0: moving statistics
    float* part;                               // scratch, p3d_stem_wgrad_part_floats() floats
    float* dw;                                 // [7][7][3][64], added to
    int chunks, chunks_per_img, chunks_per_block, pairs_per_wave, slots_per_wave, lds_row;      // set by the launcher
    int reserved_[4];
};
bool p3d_stem_wgrad_ok(int kd, int kh, int kw, int Cin, int Cout, int sd, int sh, int sw, int Wo);
long p3d_stem_wgrad_part_floats();
hipError_t p3d_stem_wgrad(const StemWgradArgs& a, int* nblocks, hipStream_t s);                   // the blocks' partials -> a.part
hipError_t p3d_stem_wgrad_fold(const float* part, int nblocks, float* dw, hipStream_t s);        // dw += the partials, in block order

#ifdef __cplusplus
}
#endif
