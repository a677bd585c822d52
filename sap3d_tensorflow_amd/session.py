"""Host-side mirror of the reference's session contract (train.py:175-218, gen_pred.py:48-64,151):
a P3DSession owns one libp3dhip handle = one built graph with its variables resident in HBM."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import P3dConfig, P3dError, P3dOpTime, check, fptr, lib
from .metrics import eval_draws

STRUCTURES = dict((name, _lib.K["P3D_STRUCTURE_" + h]) for name, h in (
    ("unet", "UNET"), ("concat", "CONCAT"), ("gn_p3d", "GN_P3D"),     # train.py:149-154 --structure
    ("unet++nonsa", "UNETPP_NONSA"),                    # p3d.py:401 p3d_unetplusplus_nonsa
    ("gn_p3d_decoder", "GN_P3D_DECODER"),               # gn/p3d_gn.py:489 inference_p3d_decoder_block (net='P3D_DECODER')
    ("gn_p3d_concat", "GN_P3D_CONCAT"),                 # gn/p3d_gn.py:279 inference_p3d_concat (net='P3D_CONCAT')
    ("unet++ds", "UNETPP_DS")))                         # p3d.py:340 p3d_unetplusplus_ds (unet++ with self attention)


def slot_names(variables, optimizer):
    """{TF slot name: (variable, slot index)} of `optimizer` ("adam" | "momentum" | "sgd") over the trainables of
    [(name, shape, trainable)]: <var>/Adam, <var>/Adam_1 (slots 0, 1) or <var>/Momentum (slot 0), as a tf.train.Saver names them."""
    out = {}
    for n, _, tr in variables:
        if tr:
            for k, suffix in enumerate(_lib.SLOT_NAMES[optimizer]):
                out["%s/%s" % (n, suffix)] = (n, k)
    return out


EMA_SUFFIX = "ExponentialMovingAverage"      # tf.train.ExponentialMovingAverage's shadow of <var>: <var>/ExponentialMovingAverage


def ema_names(variables):
    """{TF shadow name: variable} over the trainables of [(name, shape, trainable)]."""
    return dict(("%s/%s" % (n, EMA_SUFFIX), n) for n, _, tr in variables if tr)


def adam_step_from_powers(beta1_power, beta2_power, beta1=0.9, beta2=0.999):
    """Completed Adam steps t of TF's beta1_power / beta2_power (b^(t+1) as float32): the integer nearest to
    log(beta2_power) / log(beta2) - 1, checked against beta1_power (relative 1e-3, or within float32's smallest normal where
    the running product underflows).  Raises ValueError for powers that fit no step."""
    b1p, b2p = float(np.float32(beta1_power)), float(np.float32(beta2_power))
    lb1, lb2 = np.log(np.float64(np.float32(beta1))), np.log(np.float64(np.float32(beta2)))
    if not (0.0 < b2p <= 1.0) or not (lb2 < 0.0) or not (lb1 < 0.0):
        raise ValueError("beta2_power %r with beta2 %r fits no Adam step" % (b2p, beta2))
    t = int(np.rint(np.log(b2p) / lb2 - 1.0))
    if t < 0:
        raise ValueError("beta2_power %r is above beta2 %r: no Adam step" % (b2p, beta2))
    want = float(np.float32(np.float64(np.float32(beta1)) ** (t + 1)))
    if abs(b1p - want) > 1e-3 * abs(want) + float(np.finfo(np.float32).tiny):
        raise ValueError("beta1_power %r does not fit step %d of beta2_power %r (expected %r): not this optimiser's state"
                         % (b1p, t, b2p, want))
    return t


def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def _score_inputs(n, size, *maps):
    """What video_score and video_score_auc check of their maps before the library sees them: each is None or uint8 [n, H, W]
    (the shape only at a size the library takes: it refuses the rest) -> n, H, W, whether the size is one, the maps contiguous."""
    H, W = (size, size) if np.isscalar(size) else tuple(size)
    n = max(int(n), 0)
    valid = H >= 1 and W >= 1 and H * W <= 2 ** 23
    maps = [None if a is None else np.ascontiguousarray(a) for a in maps]
    for a in maps:
        if a is not None and (a.dtype != np.uint8 or (valid and a.shape != (n, H, W))):
            raise ValueError("density and fixation maps are uint8 [%d, %d, %d]" % (n, H, W))
    return n, int(H), int(W), valid, maps


def _frame_inputs(sess, n, size, frames, max_pixels, with_maps, window=None, with_out=True):
    """What video_render and video_reframe settle before the library sees the call: size (a scalar, a pair, or None for the kept
    source's or the frames' own) and frames, None or uint8 [n, H, W, 3]; then the arrays the call fills, empty at a size the
    library refuses -> n, H, W, the frames contiguous, out uint8 [n, H, W, 3] ([n] + window + [3] for a window) or None, maps
    uint8 [n, H, W] or None."""
    if size is None:
        size = sess.video_source_info()["size"] if frames is None else np.shape(frames)[1:3]
    H, W = (int(size), int(size)) if np.isscalar(size) else (int(size[0]), int(size[1]))
    n = max(int(n), 0)
    f = None
    if frames is not None:
        f = np.ascontiguousarray(frames)
        if f.dtype != np.uint8 or f.shape != (n, H, W, 3):
            raise ValueError("frames are %s %s, expected uint8 %s" % (f.dtype, f.shape, (n, H, W, 3)))
    hc, wc = (H, W) if window is None else window
    valid = H >= 1 and W >= 1 and H * W <= max_pixels and 1 <= hc <= H and 1 <= wc <= W      # (the library refuses the rest)
    out = np.empty((n, hc, wc, 3) if valid else (0,), np.uint8) if with_out else None
    maps = np.empty((n, H, W) if valid else (0,), np.uint8) if with_maps else None
    return n, H, W, f, out, maps


class P3DSession:
    """sess = P3DSession(batch=2)  ~  building the graph + tf.Session() in train.py:143-201."""

    def __init__(self, structure="unet", batch=2, frames=16, height=112, width=112, base=64, blocks=(3, 8, 36),
                 device=0, world_size=1, rank=0, seed=None):
        if structure not in STRUCTURES:
            raise ValueError("unknown structure %r (have %s)" % (structure, sorted(STRUCTURES)))
        self.cfg = P3dConfig()
        lib().p3d_default_config(C.byref(self.cfg))
        self.cfg.structure = STRUCTURES[structure]
        self.cfg.batch, self.cfg.frames, self.cfg.height, self.cfg.width = batch, frames, height, width
        self.cfg.base = base
        for i in range(3):
            self.cfg.blocks[i] = blocks[i]
        self.cfg.device, self.cfg.world_size, self.cfg.rank = device, world_size, rank
        self._h = C.c_void_p()
        check(lib().p3d_create(C.byref(self.cfg), C.byref(self._h)))
        _lib.register_session(self)
        self.x_shape = (batch, frames, height, width, 3)
        self.y_shape = (batch, frames, height, width)
        self.pred_shape = (batch, frames, height, width, 1)
        self._info = None
        self._opt = "adam"               # p3d_set_optimizer's kind, and set_adam's betas (the beta*_power of optimizer_state)
        self._betas = (0.9, 0.999)
        if seed is not None:
            self.init_params(seed)

    def close(self):
        if self._h:
            lib().p3d_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- variables (tf.global_variables / Saver) ----------------------------------------------
    def variables(self):
        """[(name, shape, trainable)] in creation order."""
        if self._info is None:
            out = []
            n = lib().p3d_num_params(self._h)
            for i in range(n):
                name = C.c_char_p()
                nd = C.c_int()
                shape = (C.c_int64 * 5)()
                tr = C.c_int()
                check(lib().p3d_param_info(self._h, i, C.byref(name), C.byref(nd), shape, C.byref(tr)))
                out.append((name.value.decode(), tuple(shape[:nd.value]), bool(tr.value)))
            self._info = out
        return self._info

    def init_params(self, seed=0):
        """tf.global_variables_initializer (train.py:178,201)."""
        check(lib().p3d_init_params(self._h, seed))

    def set_param(self, name, value):
        a = np.ascontiguousarray(value, dtype=np.float32)
        check(lib().p3d_set_param(self._h, name.encode(), fptr(a), a.size))

    def get_param(self, name):
        shape = dict((n, s) for n, s, _ in self.variables())[name]
        a = np.empty(shape, np.float32)
        check(lib().p3d_get_param(self._h, name.encode(), fptr(a), a.size))
        return a

    def get_grad(self, name):
        shape = dict((n, s) for n, s, _ in self.variables())[name]
        a = np.empty(shape, np.float32)
        check(lib().p3d_get_grad(self._h, name.encode(), fptr(a), a.size))
        return a

    def load(self, params):
        """saver.restore: {tf variable name: array}."""
        names = set(n for n, _, _ in self.variables())
        missing = names - set(params)
        if missing:
            raise KeyError("checkpoint lacks %d variables, e.g. %s" % (len(missing), sorted(missing)[:3]))
        for n in names:
            self.set_param(n, params[n])

    def restore(self, path, optimizer_state=False, ema=False, ema_as_weights=False):
        """saver.restore (train.py:204-210, gen_pred.py:57-64): `path` is a TF-1.x checkpoint prefix (`.../p3d_1000.ckpt`),
        a directory holding a `checkpoint` state file (the newest bundle is taken), or an .npz keyed by variable names.
        Variables the checkpoint lacks raise; extra ones (e.g. Adam slots of another trainer) are ignored.  With
        optimizer_state the current optimiser's slots (and Adam's beta*_power) come back too (load_optimizer_state).
        ema (set_ema must be on): the shadows come back from <var>/ExponentialMovingAverage; a checkpoint that lacks any raises,
        listing them, before anything is set.  ema_as_weights: every trainable is loaded from its shadow entry and the rest as
        usual, as a Saver over ema.variables_to_restore() does for evaluation; it needs no set_ema."""
        import os
        from . import tf_checkpoint as tfc
        if os.path.isdir(path):
            latest = tfc.latest_checkpoint(path)
            if latest is None:
                raise FileNotFoundError("no `checkpoint` state file in %s" % path)
            path = latest
        names = set(n for n, _, _ in self.variables())
        if optimizer_state:
            names |= set(self._slot_names()) | ({"beta1_power", "beta2_power"} if self._opt == "adam" else set())
        if ema and ema_as_weights:
            raise ValueError("restore: ema loads the shadows beside the weights, ema_as_weights in their place; choose one")
        shadows = ema_names(self.variables()) if (ema or ema_as_weights) else {}
        names |= set(shadows)
        if path.endswith(".npz"):
            d = dict(np.load(path))
        else:
            d = tfc.read_checkpoint(path, names=names)
        if shadows:
            missing = sorted(k for k in shadows if k not in d)
            if missing:
                raise KeyError("checkpoint lacks %d moving averages, e.g. %s" % (len(missing), missing[:3]))
        if optimizer_state:
            self._parse_optimizer_state(d)      # refuses a checkpoint without this optimiser's state before anything is set
        if ema_as_weights:
            d = dict(d)
            for k, n in shadows.items():
                d[n] = d[k]
        self.load(d)
        if optimizer_state:
            self.load_optimizer_state(d)
        if ema:
            for k, n in shadows.items():
                self.set_ema_var(n, d[k])
        return path

    def save_checkpoint(self, directory, step, keep=10, optimizer_state=False, ema=False):
        """saver.save(sess, '<dir>/p3d_<step>.ckpt') with max_to_keep (train.py:180-185,266-267): writes a TF V2 bundle and
        updates the directory's `checkpoint` state file.  With optimizer_state the bundle also holds the optimiser's slots
        under their TF names (optimizer_state()), as a default tf.train.Saver writes them; with ema the moving averages of
        set_ema under <var>/ExponentialMovingAverage (ema_state()).  Returns the prefix."""
        import os
        from . import tf_checkpoint as tfc
        prefix = os.path.join(directory, "p3d_%d.ckpt" % step)
        variables = self.save()
        if optimizer_state:
            variables.update(self.optimizer_state())
        if ema:
            variables.update(self.ema_state())
        tfc.write_checkpoint(prefix, variables)
        tfc.update_checkpoint_state(directory, prefix, keep)
        return prefix

    def save(self):
        """saver.save: {tf variable name: array} of trainables + moving statistics (train.py:180-185)."""
        return dict((n, self.get_param(n)) for n, _, _ in self.variables())

    # ---- sess.run equivalents --------------------------------------------------------------------
    def _x(self, x):
        a = np.ascontiguousarray(x, dtype=np.float32)
        if a.shape != self.x_shape:
            raise ValueError("x has shape %s, graph was built for %s" % (a.shape, self.x_shape))
        return a

    def _y(self, y):
        a = np.ascontiguousarray(y, dtype=np.float32)
        if a.shape != self.y_shape:
            raise ValueError("y has shape %s, graph was built for %s" % (a.shape, self.y_shape))
        return a

    def forward(self, x, dropout=0.0, training=False, seed=0):
        """sess.run(pred, {x, dropout, training})  (train.py:225-226, gen_pred.py:151)."""
        x = self._x(x)
        pred = np.empty(self.pred_shape, np.float32)
        check(lib().p3d_forward(self._h, fptr(x), int(bool(training)), float(dropout), seed, fptr(pred)))
        return pred

    def block_shapes(self, block_id):
        """(input shape, output shape) of bottleneck `block_id` inside this graph."""
        ishape, oshape = (C.c_int64 * 5)(), (C.c_int64 * 5)()
        check(lib().p3d_block_info(self._h, int(block_id), ishape, oshape))
        return tuple(ishape), tuple(oshape)

    def block_forward(self, block_id, x):
        """Bottleneck `block_id` of this graph in isolation (p3d.py:83-136) on input x [B,D,H,W,inplanes]."""
        ishape, oshape = self.block_shapes(block_id)
        a = np.ascontiguousarray(x, dtype=np.float32)
        if a.shape != ishape:
            raise ValueError("block %d takes %s, got %s" % (block_id, ishape, a.shape))
        out = np.empty(oshape, np.float32)
        check(lib().p3d_block_forward(self._h, int(block_id), fptr(a), a.size, fptr(out), out.size))
        return out

    def block_backward(self, block_id, x, dout):
        """Bottleneck `block_id` in isolation, forward then backward: -> gradient of its input; the block's own variables'
        gradients are then readable with get_grad."""
        ishape, oshape = self.block_shapes(block_id)
        a = np.ascontiguousarray(x, dtype=np.float32)
        d = np.ascontiguousarray(dout, dtype=np.float32)
        if a.shape != ishape or d.shape != oshape:
            raise ValueError("block %d takes %s and returns %s" % (block_id, ishape, oshape))
        din = np.empty(ishape, np.float32)
        check(lib().p3d_block_backward(self._h, int(block_id), fptr(a), a.size, fptr(d), d.size, fptr(din)))
        return din

    def schedule(self, dropout=0.5, seed=0):
        """One train step on the resident inputs, returned as the list of stream operations it issued (p3d_debug_schedule; tests)."""
        import ctypes as C
        cap = 1 << 22
        buf = C.create_string_buffer(cap)
        need = C.c_int64(0)
        check(lib().p3d_debug_schedule(self._h, float(dropout), int(seed), buf, cap, C.byref(need)))
        if need.value > cap:
            raise P3dError("schedule text of %d bytes does not fit" % need.value)
        return buf.value.decode().splitlines()

    PERTURB_MODES = {"off": 0, "serial": 1, "slow": 2}
    PERTURB_STREAMS = {"main": 0, "side": 1, "comm": 2}

    def perturb(self, mode="off", stream=None, delay_us=200):
        """Perturb the schedule of every later call of this thread on this session (p3d_debug_perturb; tests): "serial"
        synchronises the issuing stream after every launch, fill and all-reduce; "slow" puts a bounded delay kernel of delay_us
        microseconds onto `stream` ("main" | "side" | "comm") ahead of everything issued there; "off" ends it.  Results must not
        change by a bit (tests/test_gpu_stream_hazards.py)."""
        if mode not in self.PERTURB_MODES:
            raise ValueError("perturb mode %r: have %s" % (mode, sorted(self.PERTURB_MODES)))
        if mode == "slow" and stream not in self.PERTURB_STREAMS:
            raise ValueError("perturb stream %r: have %s" % (stream, sorted(self.PERTURB_STREAMS)))
        check(lib().p3d_debug_perturb(self._h, self.PERTURB_MODES[mode], self.PERTURB_STREAMS.get(stream, 0), int(delay_us)))

    def perturb_count(self):
        """(delays, syncs) inserted since the last perturb()."""
        d, s = C.c_int64(0), C.c_int64(0)
        check(lib().p3d_debug_perturb_count(self._h, C.byref(d), C.byref(s)))
        return d.value, s.value

    def decisions(self):
        """The ReLU gates and max-pool inputs of the last forward pass, as the backward pass of this session uses them
        (p3d_debug_decision_*; tests): {'relu': {BatchNorm scope: bool array [N,D,H,W,C]}, 'pool': [float32 arrays]} -- the `pins`
        an oracle evaluation takes to differentiate the same piecewise-linear branch."""
        import ctypes as C
        out = {"relu": {}, "pool": [], "relu_sites": 0}
        n = lib().p3d_debug_decision_count(self._h)
        for i in range(n):
            kind, n1, n2 = C.c_char_p(), C.c_char_p(), C.c_char_p()
            shape = (C.c_int64 * 5)()
            check(lib().p3d_debug_decision_info(self._h, i, C.byref(kind), C.byref(n1), C.byref(n2), shape))
            shp = tuple(int(v) for v in shape)
            a = np.empty(shp, np.float32)
            if kind.value == b"pool":
                check(lib().p3d_debug_decision_get(self._h, i, fptr(a), None, a.size))
                out["pool"].append(a)
                continue
            b = np.empty(shp, np.float32)
            check(lib().p3d_debug_decision_get(self._h, i, fptr(a), fptr(b), a.size))
            out["relu_sites"] += 1
            out["relu"][n1.value.decode()] = a != 0
            if n2.value:
                out["relu"][n2.value.decode()] = b != 0
        return out

    def set_pointwise_fp16(self, enable=True):
        """BASELINE configs[4]: 1x1x1 convs on the fp16 matrix cores (fp32 accumulate, fp32 storage); fp16-level parity."""
        check(lib().p3d_set_pointwise_fp16(self._h, int(bool(enable))))

    def set_bn_fusion(self, enable=True):
        """BatchNorm + ReLU between the convs of a bottleneck on the convs' operand paths (default) or as passes of their own."""
        check(lib().p3d_set_bn_fusion(self._h, int(enable)))      # 0 off, 1 forward, 2 forward + backward

    def set_attention_mode(self, mode="auto"):
        """How attention() (utils/network.py:183-185) runs: "gemm" stores the score matrix, "flash" recomputes score tiles on
        chip, "auto" picks per block by the size of the score matrix."""
        check(lib().p3d_set_attention_mode(self._h, {"auto": 0, "gemm": 1, "flash": 2}[mode]))

    def set_loss(self, name="smooth_l1", kld_weight=None, cc_weight=None, nss_weight=None, sim_weight=None):
        """The training loss of train_step / backward / train_step_device / profile_step: "smooth_l1" (the reference's,
        train.py:159; default), "bce" (sigmoid cross-entropy on the head's logits, summed; no reference counterpart -- on the
        heads without a sigmoid the raw output is taken as the logits), "l1" (L1 sum, the reference's train.py:160), or the
        per-map saliency losses "kld" (KL divergence of each [H, W] map, utils/metrics.py:338-361) and "kld_cc" (KL + (1 - CC),
        utils/metrics.py:227-250), summed over the maps with the weights of _lib.MAP_LOSSES unless kld_weight / cc_weight are
        given.  The per-map losses read the heads without a sigmoid through one (include/p3d_hip.h P3D_LOSS_KLD_CC).
        "kld_cc_nss" and "kld_cc_nss_sim" (_lib.SALIENCY_LOSSES; include/p3d_hip.h P3D_LOSS_SALIENCY) add -NSS
        (utils/metrics.py:200-224) and 1 - SIM (:258-287) per map, with nss_weight / sim_weight as further overrides; while the
        NSS weight is above 0 every train_step / backward needs the batch's fixation maps (fixations=, or upload_fixations)."""
        if name in _lib.SALIENCY_LOSSES:
            given = (kld_weight, cc_weight, nss_weight, sim_weight)
            w = [d if g is None else g for d, g in zip(_lib.SALIENCY_LOSSES[name], given)]
            try:
                w = [float(v) for v in w]
            except (TypeError, ValueError):
                raise ValueError("loss weights must be numbers, not %r" % (given,))
            if not all(np.isfinite(v) and v >= 0 for v in w) or not any(w):
                raise ValueError("loss weights must be finite, not negative and not all 0: %r" % (w,))
            check(lib().p3d_set_saliency_weights(self._h, *w))
            check(lib().p3d_set_loss(self._h, _lib.P3D_LOSS_SALIENCY))
            return
        if nss_weight is not None or sim_weight is not None:
            raise ValueError("loss %r has no NSS or SIM weight (they are for %s)" % (name, sorted(_lib.SALIENCY_LOSSES)))
        if name in _lib.MAP_LOSSES:
            kw, cw = _lib.MAP_LOSSES[name]
            kw = kw if kld_weight is None else kld_weight
            cw = cw if cc_weight is None else cc_weight
            try:
                kw, cw = float(kw), float(cw)
            except (TypeError, ValueError):
                raise ValueError("loss weights must be numbers, not %r, %r" % (kld_weight, cc_weight))
            if not (np.isfinite(kw) and np.isfinite(cw)) or kw < 0 or cw < 0 or (kw == 0 and cw == 0):
                raise ValueError("loss weights must be finite, not negative and not both 0: %r, %r" % (kw, cw))
            check(lib().p3d_set_loss_weights(self._h, kw, cw))
            check(lib().p3d_set_loss(self._h, _lib.P3D_LOSS_KLD_CC))
            return
        if name not in _lib.LOSSES:
            raise ValueError("loss %r: have %s" % (name, sorted(_lib.LOSSES) + sorted(_lib.MAP_LOSSES) + sorted(_lib.SALIENCY_LOSSES)))
        if kld_weight is not None or cc_weight is not None:
            raise ValueError("loss %r has no weights (they are for %s)" % (name, sorted(_lib.MAP_LOSSES) + sorted(_lib.SALIENCY_LOSSES)))
        check(lib().p3d_set_loss(self._h, _lib.LOSSES[name]))

    def set_regularization(self, terms=("weightdecay",), wd=None, l2=None):
        """Regularisation terms added to the training loss, the reference's two collections that its loss leaves out
        (train.py:161, gn/train_p3d_gn_dataset.py:188-189): "weightdecay" (mean over the get_conv_weight kernels of
        wd * l2_loss(w); wd defaults to 0.001 on the BatchNorm nets, 0.0005 on the GroupNorm nets) and "l2" (mean over the
        kernel_regularizer kernels of scope P3D of 0.0005 * l2_loss(w); gn_p3d_decoder only, refused elsewhere).  terms=() or
        None switches them off, the default.  The loss train_step / backward report is the data loss plus the term."""
        names = () if terms is None else ((terms,) if isinstance(terms, str) else tuple(terms))
        mask = 0
        for t in names:
            if t not in _lib.REGULARIZATION:
                raise ValueError("regularization %r: have %s" % (t, sorted(_lib.REGULARIZATION)))
            mask |= _lib.REGULARIZATION[t]
        check(lib().p3d_set_regularization(self._h, mask, float(wd or 0.0), float(l2 or 0.0)))

    def last_regularization(self):
        """The regularisation term of the last train step or backward, in double (0.0 when off); the reported loss
        includes it once per rank."""
        t = C.c_double()
        check(lib().p3d_last_regularization(self._h, C.byref(t)))
        return t.value

    def param_regularization(self, name):
        """(c_wd, c_l2): the float32 coefficients whose sum times the variable the regularisation adds to its gradient."""
        a, b = C.c_float(), C.c_float()
        check(lib().p3d_param_regularization(self._h, name.encode(), C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_grad_clip(self, clip_norm):
        """Clip the gradients of every train step by their global norm, as tf.clip_by_global_norm ahead of apply_gradients
        (an addition: the reference trains with Adam alone).  The norm is taken over every trainable element of the gradient the
        optimiser is about to apply (with the regularisation's part when that is on), in double, in a fixed order; the update
        runs on float32(g * scale), scale = float32(clip_norm / max(norm, clip_norm)), which is exactly 1 while the norm stays
        under the threshold.  float("inf") measures only; 0 (or None) switches the option off, the default.  last_grad_norm()
        reads the step's values."""
        cn = 0.0 if clip_norm is None else float(clip_norm)
        if not cn >= 0.0:
            raise ValueError("clip_norm %r: 0 (off), a positive number or inf" % (clip_norm,))
        check(lib().p3d_set_grad_clip(self._h, cn))

    def last_grad_norm(self, with_sumsq=False):
        """(norm, scale) of the last train step or backward with set_grad_clip on: the float64 global norm and the float32
        factor the step applied (backward applies none); (norm, scale, sumsq) with_sumsq.  Raises while the option is off or
        before the first step."""
        ss, nm, sc = C.c_double(), C.c_double(), C.c_float()
        check(lib().p3d_get_grad_norm(self._h, C.byref(ss), C.byref(nm), C.byref(sc)))
        return (nm.value, sc.value, ss.value) if with_sumsq else (nm.value, sc.value)

    # ---- gradient accumulation over micro-batches (p3d_set_grad_accum) ----------------------------------
    def set_grad_accum(self, k):
        """Accumulate the gradients of k micro-batches before one optimiser update (an addition: the reference updates on every
        batch of 2).  k = 1 switches the option off, the default.  With k >= 2 every train_step is one micro-step: the first
        k - 1 of a cycle run forward (moving statistics updated), loss and backward and add the gradient into an accumulator
        in float32, in the fixed order ((g0 + g1) + g2) + ...; they return the micro-batch's data loss and move neither the
        weights nor the optimiser's step.  The k-th applies the SUM (not the mean) through the usual all-reduce,
        regularisation term, clipping, optimiser and moving average.  Any call, also with the same k, discards a partial sum;
        so does init_params.  Checkpoints hold no partial sum: save when grad_accum[1] == 0."""
        check(lib().p3d_set_grad_accum(self._h, int(k)))

    @property
    def grad_accum(self):
        """(k, pending): the setting, and the micro-steps accumulated since the last update (0 .. k-1)."""
        k, pending = C.c_int(0), C.c_int(0)
        check(lib().p3d_get_grad_accum(self._h, C.byref(k), C.byref(pending)))
        return k.value, pending.value

    # ---- clip augmentation on the device (p3d_set_augment) ----------------------------------------------
    def set_augment(self, flip=0., reverse=0., min_scale=1., contrast=0., brightness=0.):
        """Augment every clip of train_step on the device (an addition: the reference's loader only resizes).  Per clip, one set
        of decisions for x, y and -- when the loss reads them -- the fixation maps: a random window of min_scale .. 1 of the
        frame resized back to H x W (cv2.INTER_LINEAR in float32; fixations by fixations_to_grid's law), a horizontal flip with
        probability `flip`, a temporal reversal with probability `reverse`, and on x alone x * a + b with a in 1 +- contrast and
        b in +- brightness.  The decisions follow from train_step's seed and the clip's global index (include/p3d_hip.h), so a
        run can be replayed; last_augment() returns them.  set_augment(None), or the defaults, switch the option off.  backward,
        forward, predict_windows, evaluate, train_step_device and profile_step never augment: forward(x) after a train_step(x, ..)
        scores the clip as given, not the augmented one; augment_inputs(seed) is the explicit form for uploaded inputs."""
        if flip is None:
            check(lib().p3d_set_augment(self._h, None))
            return
        cfg = _lib.P3dAugment(float(flip), float(reverse), float(min_scale), float(contrast), float(brightness))
        check(lib().p3d_set_augment(self._h, C.byref(cfg)))

    @property
    def augment(self):
        """None while the option is off, else dict(flip, reverse, min_scale, contrast, brightness) as float32 holds them."""
        cfg, on = _lib.P3dAugment(), C.c_int(0)
        check(lib().p3d_get_augment(self._h, C.byref(cfg), C.byref(on)))
        if not on.value:
            return None
        return dict(flip=cfg.p_flip, reverse=cfg.p_reverse, min_scale=cfg.min_scale, contrast=cfg.contrast, brightness=cfg.brightness)

    def last_augment(self):
        """The decisions of the last augmented train_step / augment_inputs, one dict per clip of this rank: flip, reverse (bool),
        y0, x0, ch, cw (the window), a, b (x * a + b).  Raises while the option is off or before the first augmentation."""
        B = self.x_shape[0]
        geom, photo = np.empty((B, 6), np.int32), np.empty((B, 2), np.float32)
        check(lib().p3d_last_augment(self._h, geom.ctypes.data_as(C.POINTER(C.c_int32)), fptr(photo)))
        return [dict(flip=bool(g[0]), reverse=bool(g[1]), y0=int(g[2]), x0=int(g[3]), ch=int(g[4]), cw=int(g[5]), a=p[0], b=p[1])
                for g, p in zip(geom, photo)]

    def last_augment_ms(self):
        """HIP-event time of the last augmentation's launches, in milliseconds."""
        ms = C.c_double()
        check(lib().p3d_last_augment_ms(self._h, C.byref(ms)))
        return ms.value

    def augment_inputs(self, seed=0):
        """Transform the uploaded inputs (upload) in place with the decisions of `seed`, once: augment_inputs(seed) followed by
        train_step_device(.., seed) is train_step(x, y, .., seed)."""
        check(lib().p3d_augment_inputs(self._h, int(seed)))

    # ---- smoothing and normalisation of the output maps (p3d_set_postprocess) ---------------------------
    def set_postprocess(self, sigma=0., radius=0, norm="none"):
        """Smooth and normalise every map that evaluate scores and pred_maps_u8 writes, at output resolution on the device (an
        addition: gen_pred.py writes map * 255 and test.py scores the bare resize).  The float32 resize, then a Gaussian of
        `sigma` pixels -- radius 0 follows cv2's rule, (int(rint(8 sigma + 1)) | 1) // 2, at most 255 -- with reflect-101 borders,
        then per map norm="max" (v / max) or "range" ((v - min) / (max - min)); include/p3d_hip.h holds the exact arithmetic and
        dataflow.postprocess_maps runs it on supplied maps.  While on, pred_maps_u8 resizes in float32 (not float64) before it
        smooths.  set_postprocess(None), or the defaults, switch the option off.  Training never sees it."""
        if sigma is None:
            check(lib().p3d_set_postprocess(self._h, None))
            return
        if norm not in _lib.NORMS:
            raise ValueError("normalisation %r: have %s" % (norm, sorted(_lib.NORMS)))
        cfg = _lib.P3dPostprocess(float(sigma), int(radius), _lib.NORMS[norm])
        check(lib().p3d_set_postprocess(self._h, C.byref(cfg)))

    @property
    def postprocess(self):
        """None while the option is off, else dict(sigma, radius, norm) as set."""
        cfg, on = _lib.P3dPostprocess(), C.c_int(0)
        check(lib().p3d_get_postprocess(self._h, C.byref(cfg), C.byref(on)))
        if not on.value:
            return None
        return dict(sigma=cfg.sigma, radius=cfg.radius, norm=[k for k, v in _lib.NORMS.items() if v == cfg.norm][0])

    # ---- histogram matching of the output maps (p3d_set_hist_match) -------------------------------------
    def set_hist_match(self, target="off", nbins=256):
        """Match the histogram of every map that evaluate scores and pred_maps_u8 / video_maps_u8 write to a target's, at output
        resolution on the device (the reference's utils/metric_utils.py match_hist; include/p3d_hip.h holds the exact arithmetic,
        dataflow.match_hist runs it on supplied maps).  target: "off" (or None); a table (cdf, bin_centers) of float64 [nt] each,
        e.g. dataflow.cumulative_distribution of a map or a pooled dataset table -- every map is matched to it; or "density":
        evaluate only, each prediction is matched to its own ground-truth density map (pred_maps_u8 and video_maps_u8 refuse
        while it is set).  `nbins` bins of the map's own histogram, 2 .. 1024.  The stage runs after set_postprocess's blur and
        before its normalisation; separate from that setting.  Training never sees it."""
        from .dataflow import _match_cfg
        cfg, keep = _match_cfg(target, nbins)
        check(lib().p3d_set_hist_match(self._h, C.byref(cfg)))

    @property
    def hist_match(self):
        """None while the option is off, else dict(mode="density" | "table", nbins) and, for a table, cdf and bin_centers."""
        cfg = _lib.P3dHistMatch()
        check(lib().p3d_get_hist_match(self._h, C.byref(cfg)))
        if cfg.mode == _lib.MATCH_MODES["off"]:
            return None
        out = dict(mode=[k for k, v in _lib.MATCH_MODES.items() if v == cfg.mode][0], nbins=cfg.nbins)
        if cfg.nt:
            out["cdf"] = np.array(cfg.cdf[:cfg.nt], np.float64)
            out["bin_centers"] = np.array(cfg.centres[:cfg.nt], np.float64)
        return out

    # ---- KL divergence and information gain of the evaluation pass (p3d_set_eval_extra) -----------------
    def set_eval_extra(self, kldiv=True, info_gain=False, baseline=None):
        """Score KL divergence (the reference's utils/metrics.py KLdiv) and / or information gain over `baseline` (the MIT
        benchmark's InfoGain; float32 [H, W] at the fixation maps' size, e.g. a centre prior or the mean training density) in
        every evaluate, at scoring resolution on the device: one more launch on the map the other metrics score
        (include/p3d_hip.h holds the arithmetic).  baseline="prior": the session's own prior (finish_prior / set_prior_map),
        copied on the device; information gain is then on.  evaluate returns what it returns; last_eval_extra() has the two
        numbers per clip.  set_eval_extra(False) switches the option off, the default.  Training never sees it."""
        if isinstance(baseline, str):
            if baseline != "prior":
                raise ValueError("baseline %r: a [H, W] map or 'prior'" % (baseline,))
            check(lib().p3d_set_eval_extra_prior(self._h, (_lib.EVAL_EXTRA["kldiv"] if kldiv else 0) | _lib.EVAL_EXTRA["info_gain"]))
            return
        flags = (_lib.EVAL_EXTRA["kldiv"] if kldiv else 0) | (_lib.EVAL_EXTRA["info_gain"] if info_gain else 0)
        base, H, W = None, 0, 0
        if baseline is not None:
            base = np.ascontiguousarray(baseline, dtype=np.float32)
            if base.ndim != 2:
                raise ValueError("the baseline is one [H, W] map")
            H, W = base.shape
        check(lib().p3d_set_eval_extra(self._h, flags, fptr(base) if base is not None else None, H, W))

    @property
    def eval_extra(self):
        """None while the option is off, else dict(kldiv, info_gain, baseline: float32 [H, W] or None)."""
        flags, H, W = C.c_int(0), C.c_int(0), C.c_int(0)
        p = C.POINTER(C.c_float)()
        check(lib().p3d_get_eval_extra(self._h, C.byref(flags), C.byref(p), C.byref(H), C.byref(W)))
        if not flags.value:
            return None
        base = np.ctypeslib.as_array(p, shape=(H.value, W.value)).copy() if p else None
        return dict(kldiv=bool(flags.value & _lib.EVAL_EXTRA["kldiv"]), info_gain=bool(flags.value & _lib.EVAL_EXTRA["info_gain"]),
                    baseline=base)

    def last_eval_extra(self):
        """[B, 2] float64: KL divergence and information gain of every clip of the last evaluate (NaN for the one that is off).
        Raises while the option is off, before an evaluate has run with it, and after an evaluate at another size than the
        baseline's."""
        out = np.empty((self.x_shape[0], 2), np.float64)
        check(lib().p3d_last_eval_extra(self._h, out.ctypes.data_as(_lib._dp), out.size))
        return out

    # ---- fixation priors (p3d_prior_*, p3d_set_prior_stage) ---------------------------------------------
    def open_prior(self, size, kind="fixations"):
        """A zeroed accumulator of size = (H, W) counts on the device (an addition: the MIT benchmark's information-gain baseline,
        the other images' fixation maps summed and smoothed).  kind "fixations": a map adds 1 where its byte is >= 128;
        "bytes": it adds the byte, for 8-bit densities.  include/p3d_hip.h holds the arithmetic.  Training never sees it."""
        if kind not in _lib.PRIOR_KINDS:
            raise ValueError("prior kind %r: have %s" % (kind, sorted(_lib.PRIOR_KINDS)))
        H, W = (size, size) if np.isscalar(size) else tuple(size)
        check(lib().p3d_prior_open(self._h, int(H), int(W), _lib.PRIOR_KINDS[kind]))

    def close_prior(self):
        """Free the accumulator; a finished prior stays."""
        check(lib().p3d_prior_close(self._h))

    def prior_info(self):
        """dict(size=(H, W), kind, n_maps) of the open accumulator."""
        H, W, k, n = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int64(0)
        check(lib().p3d_prior_info(self._h, C.byref(H), C.byref(W), C.byref(k), C.byref(n)))
        return dict(size=(H.value, W.value), kind=[q for q, v in _lib.PRIOR_KINDS.items() if v == k.value][0], n_maps=n.value)

    def prior_add(self, maps, sign=1):
        """Count uint8 maps [n, H, W] or [H, W] into the accumulator; sign=-1 takes maps out again (a leave-one-out baseline)."""
        m = np.asarray(maps)
        if m.dtype != np.uint8:
            raise ValueError("prior maps are uint8 images")
        m = np.ascontiguousarray(m[None] if m.ndim == 2 else m)
        if m.ndim != 3 or m.size == 0:
            raise ValueError("expected [n, H, W] or [H, W] uint8 maps")
        if m.shape[1:] != self.prior_info()["size"]:
            raise ValueError("the maps are %s, the accumulator %s" % (m.shape[1:], self.prior_info()["size"]))
        if sign not in (1, -1):
            raise ValueError("sign is +1 or -1")
        check(lib().p3d_prior_add(self._h, m.ctypes.data_as(_lib._u8p), m.shape[0], int(sign)))

    def prior_counts(self):
        """(uint32 [H, W] counts, the number of maps in them)."""
        H, W = self.prior_info()["size"]
        out, n = np.empty((H, W), np.uint32), C.c_int64(0)
        check(lib().p3d_prior_counts(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(n)))
        return out, n.value

    def finish_prior(self, sigma=0., radius=0):
        """Turn the counts into the session's prior: float32(count), set_postprocess's Gaussian (sigma, radius), then / max ->
        float32 [H, W], 1 at the peak; it stays on the device for set_prior_stage and set_eval_extra(baseline="prior")."""
        H, W = self.prior_info()["size"]
        out = np.empty((H, W), np.float32)
        check(lib().p3d_prior_finish(self._h, float(sigma), int(radius), fptr(out)))
        return out

    def prior_last_ms(self):
        """(ms of the last prior_add's count launches, ms of the last finish_prior's launches), by HIP events."""
        ms = (C.c_double * 2)()
        check(lib().p3d_prior_last_ms(self._h, ms))
        return ms[0], ms[1]

    def set_prior_map(self, prior):
        """Supply the prior from the host instead: float32 [H, W], finite and not constant.  None drops it."""
        if prior is None:
            check(lib().p3d_set_prior_map(self._h, None, 0, 0))
            return
        g = np.ascontiguousarray(prior, dtype=np.float32)
        if g.ndim != 2:
            raise ValueError("the prior is one [H, W] map")
        check(lib().p3d_set_prior_map(self._h, fptr(g), g.shape[0], g.shape[1]))

    @property
    def prior_map(self):
        """The session's prior, float32 [H, W], or None."""
        H, W = C.c_int(0), C.c_int(0)
        check(lib().p3d_get_prior_map(self._h, None, 0, C.byref(H), C.byref(W)))
        if H.value == 0:
            return None
        out = np.empty((H.value, W.value), np.float32)
        check(lib().p3d_get_prior_map(self._h, fptr(out), out.size, None, None))
        return out

    def set_prior_stage(self, mode="off", weight=0.):
        """Combine every map that evaluate scores and pred_maps_u8 / video_maps_u8 write with the session's prior g, at output
        resolution on the device, after set_postprocess's blur and before set_hist_match's stage.  mode "mul": v * ((1 - a) g + a)
        -- a gain of a where nothing was ever fixated, 1 at the peak; "mix": (1 - a) v + a g; a = weight in [0, 1].  "off" (or
        None) switches the stage off, the default.  Training never sees it."""
        mode = "off" if mode is None else mode
        if mode not in _lib.PRIOR_MODES:
            raise ValueError("prior mode %r: have %s" % (mode, sorted(_lib.PRIOR_MODES)))
        if mode != "off" and not 0. <= float(weight) <= 1.:
            raise ValueError("the prior weight must be in [0, 1]")
        check(lib().p3d_set_prior_stage(self._h, _lib.PRIOR_MODES[mode], float(weight)))

    @property
    def prior_stage(self):
        """None while the stage is off, else dict(mode, weight)."""
        m, a = C.c_int(0), C.c_float(0)
        check(lib().p3d_get_prior_stage(self._h, C.byref(m), C.byref(a)))
        if m.value == _lib.PRIOR_MODES["off"]:
            return None
        return dict(mode=[k for k, v in _lib.PRIOR_MODES.items() if v == m.value][0], weight=a.value)

    # ---- fixation pool and shuffled AUC in the evaluation pass (p3d_fixpool_*, p3d_eval_shuffled_*) ----------
    def open_fixation_pool(self, size, capacity):
        """A pool of `capacity` fixation maps of size = (H, W) on the device, one bit per pixel (an addition: the other clips'
        fixations that shuffled AUC samples from -- evaluate(shuffled=...)).  include/p3d_hip.h holds the layout.  Training never
        sees it."""
        H, W = (size, size) if np.isscalar(size) else tuple(size)
        check(lib().p3d_fixpool_open(self._h, int(H), int(W), int(capacity)))

    def close_fixation_pool(self):
        check(lib().p3d_fixpool_close(self._h))

    def fixation_pool_info(self):
        """dict(size=(H, W), capacity, words, filled) of the open pool."""
        H, W = C.c_int(0), C.c_int(0)
        cap, nw, nf = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(lib().p3d_fixpool_info(self._h, C.byref(H), C.byref(W), C.byref(cap), C.byref(nw), C.byref(nf)))
        return dict(size=(H.value, W.value), capacity=cap.value, words=nw.value, filled=nf.value)

    def fixation_pool_put(self, first, maps):
        """uint8 fixation maps [n, H, W] or [H, W] (fixated where the byte is >= 128) into slots first .. first + n - 1."""
        m = np.asarray(maps)
        if m.dtype != np.uint8:
            raise ValueError("fixation maps are uint8 images")
        m = np.ascontiguousarray(m[None] if m.ndim == 2 else m)
        if m.ndim != 3 or m.size == 0:
            raise ValueError("expected [n, H, W] or [H, W] uint8 maps")
        if m.shape[1:] != self.fixation_pool_info()["size"]:
            raise ValueError("the maps are %s, the pool %s" % (m.shape[1:], self.fixation_pool_info()["size"]))
        check(lib().p3d_fixpool_put(self._h, int(first), m.ctypes.data_as(_lib._u8p), m.shape[0]))

    def fixation_pool_get(self, first, n):
        """The packed words of slots first .. first + n - 1, uint64 [n, words] (for tests)."""
        out = np.empty((max(int(n), 0), self.fixation_pool_info()["words"]), np.uint64)
        check(lib().p3d_fixpool_get(self._h, int(first), int(n), out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    def fixation_pool_last_ms(self):
        """HIP-event times, ms: dict(pack: the last fixation_pool_put's launches, union: the last shuffled_begin's launch, select and
        score: the select and the clean moments + borji of the last evaluate(shuffled=...))."""
        ms = (C.c_double * 4)()
        check(lib().p3d_fixpool_last_ms(self._h, ms))
        return dict(pack=ms[0], union=ms[1], select=ms[2], score=ms[3])

    def shuffled_begin(self, others):
        """The union of the pool's maps others[b] (int [B, M], 1 <= M <= 64) for every clip of the batch, counted and scanned on the
        device -> n_other uint32 [B], the only thing that comes back.  Does not depend on the prediction."""
        ids = np.ascontiguousarray(others, dtype=np.int32)
        if ids.ndim != 2 or ids.shape[0] != self.x_shape[0]:
            raise ValueError("others is int [%d, M]" % self.x_shape[0])
        n_other = np.empty(ids.shape[0], np.uint32)
        check(lib().p3d_eval_shuffled_begin(self._h, ids.ctypes.data_as(_lib._ip), ids.shape[1], n_other.ctypes.data_as(C.POINTER(C.c_uint32))))
        return n_other

    def last_eval_shuffled(self):
        """(the means float64 [B] -- np.mean over the splits, as metrics.AUC_shuffled takes it --, the per-split areas [B, n_rep]) of
        the last evaluate(shuffled=...)."""
        out = np.empty((self.x_shape[0], getattr(self, "_shuffled_rep", 100)), np.float64)
        check(lib().p3d_last_eval_shuffled(self._h, out.ctypes.data_as(_lib._dp), out.size))
        return np.asarray([float(np.mean(r)) for r in out]), out

    # ---- moving average of the weights (p3d_set_ema) ---------------------------------------------------
    def set_ema(self, decay, warmup=False):
        """Keep an exponential moving average of every trainable variable, as tf.train.ExponentialMovingAverage(decay).apply(
        tf.trainable_variables()) after the train op (an addition: the reference scores single checkpoints).  After every
        train step s = s - (s - p) * om in float32, om = float32(1 - decay); warmup is TF's num_updates: the decay of step t is
        min(decay, (1 + t) / (10 + t)).  0 <= decay < 1; None switches the option off, the default.  Switching it on seeds the
        shadows with the current weights.  The step's loss and weights do not change; averaged() scores the shadows."""
        check(lib().p3d_set_ema(self._h, -1.0 if decay is None else float(decay), 1 if warmup else 0))

    def get_ema(self, name):
        shape = dict((n, s) for n, s, _ in self.variables())[name]
        a = np.empty(shape, np.float32)
        check(lib().p3d_get_ema(self._h, name.encode(), fptr(a), a.size))
        return a

    def set_ema_var(self, name, value):
        a = np.ascontiguousarray(value, dtype=np.float32)
        check(lib().p3d_set_ema_var(self._h, name.encode(), fptr(a), a.size))

    def ema_state(self):
        """{<var>/ExponentialMovingAverage: array}: the shadows under the names a tf.train.Saver stores them."""
        return dict((k, self.get_ema(n)) for k, n in ema_names(self.variables()).items())

    def ema_swap(self):
        """Exchange weights and moving averages of every trainable on the device, bit for bit; a second call restores both.
        While exchanged the session refuses train_step, backward, set_param, init_params and set_ema, and get_param returns
        the averages."""
        check(lib().p3d_ema_swap(self._h))

    def ema_swapped(self):
        return lib().p3d_ema_swapped(self._h) == 1

    def averaged(self):
        """with sess.averaged(): forward / evaluate / predict_windows / pred_maps_u8 run on the averaged weights; the weights
        come back on leaving the block, also through an exception."""
        import contextlib

        @contextlib.contextmanager
        def scope():
            self.ema_swap()
            try:
                yield self
            finally:
                self.ema_swap()
        return scope()

    def predict_windows(self, x):
        """B windows of gen_pred.py:100-168 at once: row k equals forward(x[k:k+1], training=False) of a batch-1
        session, i.e. every batch-statistics BN normalises each clip by its own statistics."""
        x = self._x(x)
        pred = np.empty(self.pred_shape, np.float32)
        check(lib().p3d_predict_windows(self._h, fptr(x), fptr(pred)))
        return pred

    def pred_maps_u8(self, first_frame, size=(1080, 960), scale=255.):
        """gen_pred.py:154-168's 8-bit images of the last prediction (predict_windows / forward), resized on the device:
        clip b gives frames first_frame[b] .. T-1 (0: the first window's 16 maps, 15: a later window's newest map, T: none)
        -> uint8 [sum(T - first_frame), H, W], in clip then frame order.  Each map is cv2.imwrite's byte image of
        cv2.resize(float64(map * scale), (W, H)) (dataflow.resize_linear_u8); under set_postprocess it is
        dataflow.postprocess_maps(map, size, ..., scale=scale) instead.  Device times of the call are left in
        `last_maps_ms` (device = resize / quantise, d2h = the copy back; milliseconds)."""
        H, W = (size, size) if np.isscalar(size) else tuple(size)
        B, T = self.x_shape[0], self.x_shape[1]
        ff = np.ascontiguousarray(first_frame, dtype=np.int32)
        if ff.shape != (B,):
            raise ValueError("first_frame needs one entry per clip (%d)" % B)
        valid = np.all((ff >= 0) & (ff <= T)) and H >= 1 and W >= 1 and H * W <= 2 ** 31 - 1
        out = np.empty((int(np.sum(T - ff.astype(np.int64))), H, W) if valid else (0,), np.uint8)     # (the library refuses the rest)
        ms = (C.c_double * 2)()
        check(lib().p3d_pred_maps_u8(self._h, ff.ctypes.data_as(_lib._ip), float(scale), int(H), int(W),
                                     out.ctypes.data_as(C.POINTER(C.c_ubyte)), ms))
        self.last_maps_ms = dict(device=ms[0], d2h=ms[1])
        return out

    # ---- resident video inference (p3d_video_*) -------------------------------------------------------------
    def open_video(self, frames, mode="newest"):
        """Keep a video of `frames` frames on the device (an addition: gen_pred.py keeps nothing there): its normalised frames
        go up once (video_put / video_put_u8), video_predict cuts windows where they are, and every frame's map stays on the
        device until video_maps / video_maps_u8 read it.  mode "newest": a frame's map comes from the first window that holds
        it (with starts 0, 1, 2, .. the reference's write-out rule); "mean": the float32 mean of every window that predicted it,
        summed in ascending window order.  Opening again replaces the video.  include/p3d_hip.h holds the exact rules."""
        if mode not in _lib.VIDEO_MODES:
            raise ValueError("video mode %r: have %s" % (mode, sorted(_lib.VIDEO_MODES)))
        check(lib().p3d_video_open(self._h, int(frames), _lib.VIDEO_MODES[mode]))

    def close_video(self):
        check(lib().p3d_video_close(self._h))

    def video_info(self):
        """dict(frames, mode, last_start) of the open video; last_start is -1 before the first video_predict."""
        f, m, l = C.c_int(), C.c_int(), C.c_int()
        check(lib().p3d_video_info(self._h, C.byref(f), C.byref(m), C.byref(l)))
        return dict(frames=f.value, mode=[k for k, v in _lib.VIDEO_MODES.items() if v == m.value][0], last_start=l.value)

    def video_put(self, first, frames):
        """Normalised float32 frames [n, H, W, 3] -> frames first .. first + n - 1 of the open video."""
        a = np.ascontiguousarray(frames, dtype=np.float32)
        if a.ndim != 4 or a.shape[1:] != self.x_shape[2:]:
            raise ValueError("frames are %s, the video takes [n, %d, %d, 3]" % (a.shape, self.x_shape[2], self.x_shape[3]))
        check(lib().p3d_video_put_frames(self._h, int(first), fptr(a), len(a)))

    def video_put_u8(self, first, bgr, mean_rgb=(90., 102., 98.)):
        """Decoded uint8 frames [n, H0, W0, 3] in cv2's BGR order, normalised on the device straight into the open video: what
        dataflow.mapf_frames(bgr, (H, W), mean_rgb) returns, bit for bit, without the trip back to the host."""
        a = np.ascontiguousarray(bgr)
        if a.dtype != np.uint8 or a.ndim != 4 or a.shape[3] != 3:
            raise ValueError("frames are %s %s, expected uint8 [n, H0, W0, 3]" % (a.dtype, a.shape))
        mean = np.ascontiguousarray(mean_rgb, dtype=np.float32)
        if mean.shape != (3,):
            raise ValueError("mean_rgb needs three values")
        check(lib().p3d_video_put_frames_u8(self._h, int(first), a.ctypes.data_as(_lib._u8p), a.shape[0], a.shape[1], a.shape[2], fptr(mean)))

    def video_predict(self, starts):
        """One forward pass on the windows that start at `starts` (1 .. batch of them, strictly ascending and after every start of
        an earlier call): cut on the device, predicted as predict_windows predicts them, folded into the video's maps."""
        st = np.ascontiguousarray(starts, dtype=np.int32)
        if st.ndim != 1:
            raise ValueError("starts is a list of window starts")
        check(lib().p3d_video_predict(self._h, st.ctypes.data_as(_lib._ip), len(st)))

    def video_predict_shots(self, starts):
        """video_predict with every window held inside its shot of the installed table (video_set_shots / video_detect_shots; an
        addition): a start is its shot's first frame or at least T - 1 frames from the shot's end (T the session's frames), a window of a
        shorter shot is filled by reflecting inside the shot, and only the frames start .. min(start + T - 1, the shot's end) take
        its maps.
        dataflow.shot_window_starts lays such windows out; include/p3d_hip.h ("Shot-aware windows") holds the exact rules."""
        st = np.ascontiguousarray(starts, dtype=np.int32)
        if st.ndim != 1:
            raise ValueError("starts is a list of window starts")
        check(lib().p3d_video_predict_shots(self._h, st.ctypes.data_as(_lib._ip), len(st)))

    def video_last_ms(self):
        """HIP-event times of the last video_predict's window cut and map fold: dict(gather, scatter), milliseconds."""
        ms = (C.c_double * 2)()
        check(lib().p3d_video_last_ms(self._h, ms))
        return dict(gather=ms[0], scatter=ms[1])

    def set_video_temporal(self, kind="off", sigma=0., radius=0, alpha=0.):
        """Smooth the open video's maps along the frame axis when they are read (an addition: overlapping 16-frame windows flicker
        from frame to frame).  kind "gauss": a Gaussian of `sigma` frames over the whole video -- radius 0 follows cv2's rule,
        (int(rint(8 sigma + 1)) | 1) // 2; at most 24, and at most frames - 1 -- with reflect-101 at the first and last frame;
        "ema": the causal m_f = alpha m_{f-1} + (1 - alpha) v_f from m_0 = v_0, alpha in [0, 1).  Under mode "mean" the input is
        sum / count.  video_maps returns the filtered maps and video_maps_u8 runs its chain on them; the stores are never
        rewritten, so more windows can follow.  include/p3d_hip.h holds the exact arithmetic and dataflow.temporal_filter runs
        it on supplied maps.  set_video_temporal("off"), None or the defaults switch it off.  Needs no open video."""
        if kind is None:
            kind = "off"
        if kind not in _lib.TEMPORAL_KINDS:
            raise ValueError("temporal kind %r: have %s" % (kind, sorted(_lib.TEMPORAL_KINDS)))
        cfg = _lib.P3dVideoTemporal(_lib.TEMPORAL_KINDS[kind], float(sigma), int(radius), float(alpha))
        check(lib().p3d_set_video_temporal(self._h, C.byref(cfg)))

    def get_video_temporal(self):
        """None while the option is off, else dict(kind, sigma, radius, alpha) as set."""
        cfg, on = _lib.P3dVideoTemporal(), C.c_int(0)
        check(lib().p3d_get_video_temporal(self._h, C.byref(cfg), C.byref(on)))
        if not on.value:
            return None
        return dict(kind=[k for k, v in _lib.TEMPORAL_KINDS.items() if v == cfg.kind][0], sigma=cfg.sigma, radius=cfg.radius, alpha=cfg.alpha)

    def video_temporal_last_ms(self):
        """HIP-event time of the temporal launch of the last video_maps / video_maps_u8 that ran the stage, milliseconds."""
        ms = C.c_double(0.)
        check(lib().p3d_video_temporal_last_ms(self._h, C.byref(ms)))
        return ms.value

    def video_maps(self, first, n, with_counts=False):
        """Maps of frames first .. first + n - 1, float32 [n, H, W] (mode "mean": sum / count); with_counts: also how many
        windows contributed to each.  A frame no window has predicted yet is refused.  Under set_video_temporal the maps are
        filtered along the frame axis of the whole video (the counts stay the frames' own), and every frame the filter needs --
        up to its radius either side, or every earlier frame for "ema" -- must have been predicted."""
        n = max(int(n), 0)
        maps = np.empty((n,) + self.y_shape[2:], np.float32)
        counts = np.zeros(n, np.int32)
        check(lib().p3d_video_get_maps(self._h, int(first), n, fptr(maps), counts.ctypes.data_as(C.POINTER(C.c_int32))))
        return (maps, counts) if with_counts else maps

    def video_maps_u8(self, first, n, size=(1080, 960), scale=255.):
        """pred_maps_u8's 8-bit images of frames first .. first + n - 1 of the open video -> uint8 [n, H, W]; under
        set_postprocess the smoothed, normalised ones.  Under set_video_temporal the maps are filtered along the frame axis first
        and the chain runs on the filtered maps.  Device times are left in `last_maps_ms`."""
        H, W = (size, size) if np.isscalar(size) else tuple(size)
        n = max(int(n), 0)
        valid = H >= 1 and W >= 1 and H * W <= 2 ** 31 - 1
        out = np.empty((n, H, W) if valid else (0,), np.uint8)     # (the library refuses the rest)
        ms = (C.c_double * 2)()
        check(lib().p3d_video_maps_u8(self._h, int(first), n, float(scale), int(H), int(W), out.ctypes.data_as(_lib._u8p), ms))
        self.last_maps_ms = dict(device=ms[0], d2h=ms[1])
        return out

    def video_score(self, first, n, density, fixation, size=(1080, 960), scale=255., columns=("cc", "sim", "judd"), ties="expected",
                    with_maps=False):
        """Score frames first .. first + n - 1 of the open video on the device (an addition: the arithmetic of the reference's
        utils/matlab_metric/metric_video_base.m protocol): video_maps_u8's bytes, where they are, against density and fixation,
        uint8 [n, H, W] at `size` (fixated: byte >= 128) -> float64 [n, 5]: CC, SIM, AUC_Judd, KL, NSS, NaN in the columns not
        named in `columns` ("cc", "sim", "judd", "kl", "nss"; "matlab" is the first three).  ties: AUC_Judd on equal bytes,
        "reference" (utils/metrics.py with jitter=False) or "expected" (its mean over every order of the tied pixels, what the
        default jitter does to an 8-bit map).  fixation may be None when neither judd nor nss is asked for.  with_maps: also the
        scored bytes, uint8 [n, H, W].  Device times are left in `last_score_ms`.  include/p3d_hip.h holds the exact rules."""
        from . import metrics
        n, H, W, valid, (dens, fix) = _score_inputs(n, size, np.ascontiguousarray(density), fixation)
        out = np.full((n, 5), np.nan, np.float64)
        maps = np.empty((n, H, W) if valid else (0,), np.uint8) if with_maps else None
        ms = (C.c_double * 3)()
        check(lib().p3d_video_score(self._h, int(first), n, float(scale), H, W, _ptr(dens, _lib._u8p), _ptr(fix, _lib._u8p),
                                    metrics.score_flags(columns), metrics.score_ties(ties), _ptr(out, _lib._dp), _ptr(maps, _lib._u8p), ms))
        self.last_score_ms = dict(upload=ms[0], device=ms[1], score=ms[2])
        return (out, maps) if with_maps else out

    def video_keep_source(self, on=True):
        """Keep the decoded frames of video_put_u8 on the device as they were put, for video_render (an addition).  Legal only
        right after open_video, before the first video_put_u8; every open_video starts with it off.  The first video_put_u8 then
        fixes the frames' size and allocates uint8 [frames, H0, W0, 3]; the normalised floats stay what they were, bit for bit."""
        check(lib().p3d_video_keep_source(self._h, 1 if on else 0))

    def video_source_info(self):
        """dict(on, size=(H0, W0) -- (0, 0) until the first video_put_u8 --, bytes) of the open video's source store."""
        on, h0, w0, b = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int64(0)
        check(lib().p3d_video_source_info(self._h, C.byref(on), C.byref(h0), C.byref(w0), C.byref(b)))
        return dict(on=bool(on.value), size=(h0.value, w0.value), bytes=b.value)

    def video_render(self, first, n, frames=None, size=None, scale=255., table=None, colormap="jet", alpha=0.6, opacity="ramp", gate=0,
                     contour=None, thickness=1, contour_color=(255, 255, 255), with_maps=False, timed=False):
        """Frames first .. first + n - 1 of the open video with their saliency maps laid over them, on the device (an addition:
        what the reference's gen_video.py is for) -> uint8 [n, H, W, 3] in B, G, R order.  The maps are video_maps_u8's bytes at
        `size`, where they are; frames: uint8 [n, H, W, 3] at that size, or None for the source kept by video_keep_source (size
        then defaults to, and must be, the source's own).  table: uint32 [256] of dataflow.render_table, or None to build it from
        colormap ("grey", "hot", "jet"), alpha, opacity ("ramp", "constant") and gate.  contour: the level whose iso-line is
        drawn `thickness` pixels wide in contour_color (R, G, B); None: no line.  with_maps: also the maps, uint8 [n, H, W].
        timed: HIP-event times are left in `last_render_ms` (upload, device = the maps' chain, render).  include/p3d_hip.h holds
        the exact rules."""
        from . import dataflow
        n, H, W, f, out, maps = _frame_inputs(self, n, size, frames, 2 ** 28, with_maps)
        cfg = dataflow.render_cfg(dataflow.render_table(colormap, alpha, opacity, gate) if table is None else table, contour, thickness,
                                  contour_color)
        ms = (C.c_double * 3)()
        check(lib().p3d_video_render(self._h, int(first), n, float(scale), H, W, _ptr(f, _lib._u8p), C.byref(cfg), _ptr(out, _lib._u8p),
                                     _ptr(maps, _lib._u8p), ms if timed else None))
        if timed:
            self.last_render_ms = dict(upload=ms[0], device=ms[1], render=ms[2])
        return (out, maps) if with_maps else out

    def video_reframe(self, first, n, crop, frames=None, size=None, scale=255., gate=0, smooth=0, with_raw=False, with_mass=False,
                      with_maps=False, timed=False):
        """Frames first .. first + n - 1 of the open video reframed around their saliency, on the device (an addition): per frame
        the crop = (hc, wc) window of the largest gated saliency mass, the track box-smoothed over `smooth` frames to either side
        WITHIN THIS CALL (ask for the whole video in one call for one track) -> dict(track int32 [n, 2] (Y, X), crop uint8
        [n, hc, wc, 3] in B, G, R order or None).  The maps are video_maps_u8's bytes at `size`, where they are.  frames: uint8
        [n, H, W, 3] at that size, None for the source kept by video_keep_source (size then defaults to, and must be, the
        source's own), or False for the tracks alone (size is then required).  with_raw / with_mass / with_maps add raw int32
        [n, 2], mass uint32 [n, 3] (best, smoothed, total) and maps uint8 [n, H, W].  timed: HIP-event times are left in
        `last_reframe_ms` (upload, device = the maps' chain, reframe).  include/p3d_hip.h holds the exact rules."""
        tracks_only = frames is False
        if tracks_only and size is None:
            raise ValueError("tracks alone (frames=False) need a size")
        hc, wc = (int(crop), int(crop)) if np.isscalar(crop) else (int(crop[0]), int(crop[1]))
        n, H, W, f, out, maps = _frame_inputs(self, n, size, None if tracks_only else frames, 2 ** 23, with_maps, (hc, wc), not tracks_only)
        cfg = _lib.P3dReframe(hc, wc, int(gate), int(smooth))
        track = np.empty((n, 2), np.int32)
        raw = np.empty((n, 2), np.int32) if with_raw else None
        mass = np.empty((n, 3), np.uint32) if with_mass else None
        ms = (C.c_double * 3)()
        check(lib().p3d_video_reframe(self._h, int(first), n, float(scale), H, W, _ptr(f, _lib._u8p), C.byref(cfg), _ptr(track, _lib._i32p),
                                      _ptr(raw, _lib._i32p), _ptr(mass, _lib._u32p), _ptr(out, _lib._u8p), _ptr(maps, _lib._u8p),
                                      ms if timed else None))
        if timed:
            self.last_reframe_ms = dict(upload=ms[0], device=ms[1], reframe=ms[2])
        res = dict(track=track, crop=out)
        if with_raw:
            res["raw"] = raw
        if with_mass:
            res["mass"] = mass
        if with_maps:
            res["maps"] = maps
        return res

    def video_regions(self, first, n, size, gate, connectivity=8, min_area=1, max_regions=None, link=False, scale=255., with_labels=False,
                      with_maps=False, timed=False):
        """The salient regions of frames first .. first + n - 1 of the open video, on the device (an addition): the connected
        regions of the pixels at or above `gate` in video_maps_u8's bytes at `size`, per frame the max_regions heaviest of at least
        min_area pixels -> dict(regions int32 [n, K, P3D_REGION_FIELDS], counts int32 [n, 3] (found, large enough, kept)).  link:
        regions carry an ID from frame to frame by overlap WITHIN THIS CALL and inside the shots of video_set_shots' table.
        with_labels / with_maps add labels uint8 [n, H, W] (a region's rank, 255 elsewhere) and maps uint8 [n, H, W].  timed: HIP-event
        times are left in `last_regions_ms` (device = the maps' chain, regions).  include/p3d_hip.h holds the exact rules."""
        from . import dataflow
        H, W = (int(size), int(size)) if np.isscalar(size) else (int(size[0]), int(size[1]))
        n = max(int(n), 0)
        K = _lib.P3D_REGIONS_MAX if max_regions is None else int(max_regions)
        valid = H >= 1 and W >= 1 and H * W <= 2 ** 23 and 1 <= K <= _lib.P3D_REGIONS_MAX      # (the library refuses the rest)
        cfg = dataflow.regions_cfg(gate, connectivity, min_area, K, link)
        rec = np.empty((n, K, _lib.P3D_REGION_FIELDS) if valid else (1,), np.int32)
        counts = np.empty((n, 3), np.int32)
        lab = np.empty((n, H, W) if valid else (0,), np.uint8) if with_labels else None
        maps = np.empty((n, H, W) if valid else (0,), np.uint8) if with_maps else None
        ms = (C.c_double * 3)()
        check(lib().p3d_video_regions(self._h, int(first), n, float(scale), H, W, cfg, _ptr(rec, _lib._i32p), _ptr(counts, _lib._i32p),
                                      _ptr(lab, _lib._u8p), _ptr(maps, _lib._u8p), ms if timed else None))
        if timed:
            self.last_regions_ms = dict(device=ms[1], regions=ms[2])
        res = dict(regions=rec, counts=counts)
        if with_labels:
            res["labels"] = lab
        if with_maps:
            res["maps"] = maps
        return res

    def video_qpmap(self, first, n, size, law, block=16, peak_weight=128, dilate=0, fall=0, rise=0, balance=True, target=0, lo=-127, hi=127,
                    scale=255., with_levels=False, with_stats=False, with_maps=False, timed=False):
        """Quantiser offsets per coding block of frames first .. first + n - 1 of the open video, on the device (an addition): the
        level of every block x block block of video_maps_u8's bytes at `size` (peak_weight / 256 of its largest byte, the rest its
        mean), dilated by `dilate` blocks, turned into an offset by `law` (int32 [256], dataflow.qp_law), limited to `fall` down and
        `rise` up per frame WITHIN THIS CALL and inside the shots of video_set_shots' table, and with `balance` shifted so that the
        frame's area-weighted mean is `target`, then clamped to [lo, hi] -> dict(qp int32 [n, Hb, Wb]).  with_levels / with_stats /
        with_maps add levels uint8 [n, Hb, Wb], stats int32 [n, 4] (min, max, S1, S2) and maps uint8 [n, H, W].  timed: HIP-event
        times are left in `last_qpmap_ms` (device = the maps' chain, qpmap).  include/p3d_hip.h holds the exact rules."""
        from . import dataflow
        H, W = (int(size), int(size)) if np.isscalar(size) else (int(size[0]), int(size[1]))
        n = max(int(n), 0)
        B = int(block)
        valid = H >= 1 and W >= 1 and H * W <= 2 ** 23 and B in dataflow.QPMAP_BLOCKS      # (the library refuses the rest)
        t = dataflow._qp_law_array(law)
        cfg = dataflow.qpmap_cfg(B, peak_weight, dilate, fall, rise, balance, target, lo, hi)
        grid = (n, -(-H // B), -(-W // B)) if valid else (1,)
        qp = np.empty(grid, np.int32)
        lev = np.empty(grid, np.uint8) if with_levels else None
        st4 = np.empty((n, 4), np.int32) if with_stats else None
        maps = np.empty((n, H, W) if valid else (0,), np.uint8) if with_maps else None
        ms = (C.c_double * 3)()
        check(lib().p3d_video_qpmap(self._h, int(first), n, float(scale), H, W, cfg, _ptr(t, _lib._i32p), _ptr(qp, _lib._i32p),
                                    _ptr(lev, _lib._u8p), _ptr(st4, _lib._i32p), _ptr(maps, _lib._u8p), ms if timed else None))
        if timed:
            self.last_qpmap_ms = dict(device=ms[1], qpmap=ms[2])
        res = dict(qp=qp)
        if with_levels:
            res["levels"] = lev
        if with_stats:
            res["stats"] = st4
        if with_maps:
            res["maps"] = maps
        return res

    def video_prefilter(self, first, n, H, W, law, block=16, peak_weight=128, dilate=0, fall=0, rise=0, radius=4, passes=1, frames=None,
                        scale=255.):
        """Frames first .. first + n - 1 of the open video low-pass filtered away from their saliency, on the device (an addition: a
        pre-filter any encoder can take) -> (out uint8 [n, H, W, 3] in B, G, R order, grid int32 [n, Hb, Wb], maps uint8 [n, H, W],
        stage_ms).  Per block x block block of video_maps_u8's bytes at H x W a strength 0 .. 64: the block's level (peak_weight /
        256 of its largest byte, the rest its mean), dilated by `dilate` blocks, turned into a strength by `law` (int32 [256],
        dataflow.prefilter_law), limited to `fall` down and `rise` up per frame WITHIN THIS CALL and inside the shots of
        video_set_shots' table.  The strength is interpolated between block centres into a weight per pixel, which blends in a
        low-pass of `passes` rounded box passes, `radius` pixels either way; where the weight is 0 the frame's bytes are returned.
        frames: uint8 [n, H, W, 3], or None for the source kept by video_keep_source (H x W must then be the source's own).
        stage_ms: dict(upload, device = the maps' chain, prefilter) of HIP-event times.  include/p3d_hip.h holds the exact rules."""
        from . import dataflow
        n, H, W, f, out, maps = _frame_inputs(self, n, (H, W), frames, 2 ** 23, True)
        B = int(block)
        valid = out.ndim == 4 and B in dataflow.QPMAP_BLOCKS      # (the library refuses the rest)
        t = dataflow._prefilter_law_array(law)
        cfg = dataflow.prefilter_cfg(B, peak_weight, dilate, fall, rise, radius, passes)
        grid = np.empty((n, -(-H // B), -(-W // B)) if valid else (1,), np.int32)
        ms = (C.c_double * 3)()
        check(lib().p3d_video_prefilter(self._h, int(first), n, float(scale), H, W, _ptr(f, _lib._u8p), cfg, _ptr(t, _lib._i32p),
                                        _ptr(out, _lib._u8p), _ptr(grid, _lib._i32p), _ptr(maps, _lib._u8p), ms))
        return out, grid, maps, dict(upload=ms[0], device=ms[1], prefilter=ms[2])

    def video_distortion(self, first, n, test, law, block=0, gate=0, ref=None, size=None, block_map=None, scale=255.):
        """Frames first .. first + n - 1 of the open video compared with `test` under their saliency, on the device (an addition: what
        a pre-filter or an encoder cost where the viewers look) -> (table int64 [n, P3D_DISTORTION_RECORD], block_sse int64
        [n, Hb, Wb] or None, maps uint8 [n, H, W], stage_ms).  test: uint8 [n, H, W, 3] in B, G, R order, the decoded or filtered
        frames.  ref: uint8 [n, H, W, 3], or None for the source kept by video_keep_source (H x W must then be the source's own).
        The weights are `law` (int32 [256], dataflow.distortion_law) of video_maps_u8's bytes at H x W; `gate` counts the salient
        pixels and those of them that changed; `block` (8 .. 128, 0: none) sizes the map of squared errors per block.  The table
        holds integers alone; dataflow.distortion_report(table, H * W) gives PSNR, weighted PSNR, SSIM and weighted SSIM.
        stage_ms: dict(upload, device = the maps' chain, distortion) of HIP-event times.  include/p3d_hip.h holds the exact rules."""
        from . import dataflow
        if test is None:
            raise ValueError("test frames are required")
        if size is None and ref is None:
            size = np.shape(test)[1:3]
        n, H, W, r, _, maps = _frame_inputs(self, n, size, ref, 2 ** 23, True, with_out=False)
        t = np.ascontiguousarray(test)
        if t.dtype != np.uint8 or t.shape != (n, H, W, 3):
            raise ValueError("test frames are %s %s, expected uint8 %s" % (t.dtype, t.shape, (n, H, W, 3)))
        B = int(block)
        w = dataflow._distortion_law_array(law)
        cfg = dataflow.distortion_cfg(B, gate)
        table = np.empty((n, _lib.P3D_DISTORTION_RECORD), np.int64)
        want_map = B != 0 if block_map is None else bool(block_map)
        valid = maps.ndim == 3 and B in dataflow.QPMAP_BLOCKS      # (the library refuses the rest)
        bs = np.empty((n, -(-H // B), -(-W // B)) if valid else (1,), np.int64) if want_map else None
        ms = (C.c_double * 3)()
        check(lib().p3d_video_distortion(self._h, int(first), n, float(scale), H, W, _ptr(r, _lib._u8p), _ptr(t, _lib._u8p), cfg,
                                         _ptr(w, _lib._i32p), _ptr(table, _lib._i64p), _ptr(bs, _lib._i64p), _ptr(maps, _lib._u8p), ms))
        return table, bs, maps, dict(upload=ms[0], device=ms[1], distortion=ms[2])

    def video_detect_shots(self, grid=(2, 2), threshold=250, window=2, ratio=512, min_length=3, install=True, with_signal=False):
        """Find the hard cuts of the open video on the device (an addition), from the source kept by video_keep_source: per frame a
        grid = (gy, gx) of cell histograms of the B, G, R bytes, D_f their distance from the frame before; frame f starts a shot
        when D_f is at least `threshold` permille of its largest possible value 6 H W, at least ratio / 256 times every other D
        within `window` frames (a flash fails this), and at least `min_length` frames from the last cut and from the end.  Returns
        the starts, int32 [n_shots] ascending from 0 (with_signal: also D, uint32 [frames]); install: the table is installed as
        video_set_shots would.  Dissolves and fades are not detected (video_detect_transitions finds them).  include/p3d_hip.h holds
        the exact rules."""
        from . import dataflow
        F = self.video_info()["frames"]
        cfg = dataflow.shots_cfg(grid, threshold, window, ratio, min_length)
        D, starts, count = np.zeros(max(F, 1), np.uint32), np.zeros(max(F, 1), np.int32), C.c_int(0)
        check(lib().p3d_video_detect_shots(self._h, cfg, _ptr(D, _lib._u32p), _ptr(starts, _lib._i32p), len(starts), C.byref(count),
                                           1 if install else 0))
        starts = starts[:count.value].copy()
        return (starts, D) if with_signal else starts

    def video_detect_transitions(self, grid=(2, 2), threshold=250, window=2, ratio=512, min_length=3, lag=12, high=250, dip=230, mono=768,
                                 mono_min=2, install=True, with_signals=False):
        """video_detect_shots with dissolves and fades (an addition): beside D_f, the distance E_f of frame f's histograms from
        frame f - lag's and the spread v_f of its bins.  A run of monochrome frames (v_f 256 <= mono H W) of at least mono_min
        frames ends a shot at its last frame (a fade); a run of E_f >= high permille of 6 H W that is lag / 2 .. 2 lag frames long,
        holds no cut and no monochrome frame and dips in v to dip / 256 of its ends starts a shot at its middle less lag / 2 (a
        dissolve).  lag = 0 switches dissolves off, mono_min = 0 fades.  Returns (starts, kinds), int32 [n_shots] each, kinds the
        P3D_SHOT_* numbers (with_signals: also D, E uint32 [frames] and v int64 [frames]); install: the table is installed as
        video_set_shots would, with its kinds (video_shot_kinds).  include/p3d_hip.h ("Gradual transitions") holds the exact rules."""
        from . import dataflow
        F = self.video_info()["frames"]
        cfg, gcfg = dataflow.shots_cfg(grid, threshold, window, ratio, min_length), dataflow.gradual_cfg(lag, high, dip, mono, mono_min)
        room = max(F, 1)
        D, E, v = np.zeros(room, np.uint32), np.zeros(room, np.uint32), np.zeros(room, np.int64)
        starts, kinds, count = np.zeros(room, np.int32), np.zeros(room, np.int32), C.c_int(0)
        check(lib().p3d_video_detect_transitions(self._h, cfg, gcfg, _ptr(D, _lib._u32p), _ptr(E, _lib._u32p), _ptr(v, _lib._i64p),
                                                 _ptr(starts, _lib._i32p), _ptr(kinds, _lib._i32p), room, C.byref(count), 1 if install else 0))
        starts, kinds = starts[:count.value].copy(), kinds[:count.value].copy()
        return (starts, kinds, D, E, v) if with_signals else (starts, kinds)

    def video_shot_kinds(self):
        """The kinds of the installed shot table, int32 [n_shots] of P3D_SHOT_* numbers, or None without a table: FIRST, then what
        video_detect_transitions found, or CUT throughout for a table of video_set_shots or video_detect_shots."""
        count = C.c_int(0)
        check(lib().p3d_video_get_shot_kinds(self._h, None, 0, C.byref(count)))
        if not count.value:
            return None
        kinds = np.empty(count.value, np.int32)
        check(lib().p3d_video_get_shot_kinds(self._h, _ptr(kinds, _lib._i32p), len(kinds), C.byref(count)))
        return kinds

    def video_set_shots(self, starts):
        """Install a shot table on the open video: starts ascending from 0, each the first frame of a shot; None removes it.  While
        one is installed, set_video_temporal's filter runs inside the shots (reflecting at their ends, the moving average restarting)
        and video_reframe smooths its track inside them; open_video starts without one."""
        if starts is None:
            check(lib().p3d_video_set_shots(self._h, None, 0))
            return
        st = np.ascontiguousarray(starts, np.int32).ravel()
        room = st if len(st) else np.zeros(1, np.int32)      # (an empty table is refused by the library, not taken for None)
        check(lib().p3d_video_set_shots(self._h, _ptr(room, _lib._i32p), len(st)))

    def video_shots(self):
        """The installed shot table, int32 [n_shots], or None."""
        count = C.c_int(0)
        check(lib().p3d_video_get_shots(self._h, None, 0, C.byref(count)))
        if not count.value:
            return None
        st = np.empty(count.value, np.int32)
        check(lib().p3d_video_get_shots(self._h, _ptr(st, _lib._i32p), len(st), C.byref(count)))
        return st

    def video_shots_last_ms(self):
        """HIP-event times of the last video_detect_shots, milliseconds: dict(signal, decision)."""
        ms = (C.c_double * 2)()
        check(lib().p3d_video_shots_last_ms(self._h, ms))
        return dict(signal=ms[0], decision=ms[1])

    def video_shuffled_begin(self, ids):
        """The union of the fixation pool's maps ids[b] (int [n, M], 1 <= M <= 64) for each of n frames that video_score_auc will
        score, counted and scanned on the device -> n_other uint32 [n].  Held apart from shuffled_begin's union: an armed
        evaluate(shuffled=...) is not disturbed."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        if ids.ndim != 2:
            raise ValueError("ids is int [n, M]")
        n_other = np.empty(ids.shape[0], np.uint32)
        check(lib().p3d_video_shuffled_begin(self._h, ids.shape[0], ids.ctypes.data_as(_lib._ip), ids.shape[1],
                                             n_other.ctypes.data_as(C.POINTER(C.c_uint32))))
        return n_other

    def video_score_auc(self, first, n, density, fixation, size=(1080, 960), scale=255., columns=("cc", "sim", "judd"), ties="expected",
                        borji_idx=None, shuffled_ranks=None, n_rows=None, n_rep=100, step_size=0.1):
        """video_score with AUC-Borji and shuffled AUC of the same bytes (include/p3d_hip.h, SPLIT SWEEP): one maps chain, one
        pass A, then everything asked for.  columns: as video_score, or () / None for none of the five (density may then be None).
        borji_idx: every frame's randint(0, H * W, [nf, n_rep]) indices, concatenated (metrics.borji_draws_u8).  shuffled_ranks,
        n_rows: metrics.shuffled_draws' ranks into the union video_shuffled_begin holds for these n frames.
        -> dict(scores float64 [n, 5], borji [n, n_rep], shuffled [n, n_rep]; NaN where not asked).  Device times are left in
        `last_score_ms`: upload, device (the maps' chain), score (the five columns), auc (preparation, select and sweeps)."""
        from . import metrics
        n, H, W, _, (dens, fix) = _score_inputs(n, size, density, fixation)
        flags = metrics.score_flags(columns if columns is not None else ())
        n_rep = int(n_rep)
        res = dict(scores=np.full((n, 5), np.nan, np.float64), borji=np.full((n, max(n_rep, 0)), np.nan, np.float64),
                   shuffled=np.full((n, max(n_rep, 0)), np.nan, np.float64))

        def ints(a):        # (a one-element array where there is nothing: NULL means "not asked")
            a = np.ascontiguousarray(a, dtype=np.int32).ravel()
            return a if a.size else np.zeros(1, np.int32)
        bi = None if borji_idx is None else ints(borji_idx)
        rk = None if shuffled_ranks is None else ints(shuffled_ranks)
        nr = None if n_rows is None else np.ascontiguousarray(n_rows, dtype=np.int32).ravel()
        if rk is not None and (nr is None or nr.size != n):
            raise ValueError("n_rows is int [%d], the rows of shuffled_ranks per frame" % n)
        ms = (C.c_double * 4)()
        check(lib().p3d_video_score_auc(self._h, int(first), n, float(scale), H, W, _ptr(dens, _lib._u8p), _ptr(fix, _lib._u8p), flags,
                                        metrics.score_ties(ties), _ptr(res["scores"] if flags else None, _lib._dp), _ptr(bi, _lib._ip),
                                        _ptr(rk, _lib._ip), _ptr(nr, _lib._ip), n_rep, float(step_size),
                                        _ptr(res["borji"] if bi is not None else None, _lib._dp),
                                        _ptr(res["shuffled"] if rk is not None else None, _lib._dp), ms))
        self.last_score_ms = dict(upload=ms[0], device=ms[1], score=ms[2], auc=ms[3])
        return res

    # ---- resident training set (p3d_trainset_*) -------------------------------------------------------------
    def open_trainset(self, frames_per_video, frame_format="u8", fixations=False, mean_rgb=(90., 102., 98.)):
        """Keep a training set on the device (an addition: the reference's loader, dataflow.py:39-62, cuts overlapping clips on
        the host): videos of frames_per_video[v] frames each, their decoded frames, density maps and -- fixations=True -- fixation
        maps go up once (trainset_put_*), and trainset_stage / trainset_step / trainset_forward cut a batch of (video, start)
        clips where they are, into the buffers a train step reads.  frame_format "u8" keeps 3 bytes per pixel and takes only
        frames decoded at the grid's size; "f32" keeps the floats of dataflow.mapf_frames, for any source size.  The staged x and y
        are what dataflow.mapf_frames(..., mean_rgb) and dataflow.mapf_density return for the clips' frames, bit for bit.
        Opening again replaces the set.  include/p3d_hip.h holds the exact rules."""
        if frame_format not in _lib.TRAINSET_FORMATS:
            raise ValueError("frame format %r: have %s" % (frame_format, sorted(_lib.TRAINSET_FORMATS)))
        fr = np.ascontiguousarray(frames_per_video, dtype=np.int32)
        if fr.ndim != 1:
            raise ValueError("frames_per_video is a list of frame counts, one per video")
        mean = np.ascontiguousarray(mean_rgb, dtype=np.float32)
        if mean.shape != (3,):
            raise ValueError("mean_rgb needs three values")
        check(lib().p3d_trainset_open(self._h, len(fr), fr.ctypes.data_as(_lib._ip), _lib.TRAINSET_FORMATS[frame_format],
                                      _lib.P3D_TRAINSET_FIXATIONS if fixations else 0, fptr(mean)))

    def close_trainset(self):
        check(lib().p3d_trainset_close(self._h))

    def trainset_info(self):
        """dict(videos, total_frames, frame_format, fixations, bytes, frames, put) of the open set: `frames` the frames of every
        video, `put` how many of them were put per video as dict(frames, density, fixations) of lists."""
        v, t, f, fl, b = C.c_int(), C.c_int64(), C.c_int(), C.c_int(), C.c_int64()
        check(lib().p3d_trainset_info(self._h, C.byref(v), C.byref(t), C.byref(f), C.byref(fl), C.byref(b)))
        frames, put = [], dict(frames=[], density=[], fixations=[])
        for i in range(v.value):
            n, a, d, x = C.c_int(), C.c_int(), C.c_int(), C.c_int()
            check(lib().p3d_trainset_video_info(self._h, i, C.byref(n), C.byref(a), C.byref(d), C.byref(x)))
            frames.append(n.value); put["frames"].append(a.value); put["density"].append(d.value); put["fixations"].append(x.value)
        return dict(videos=v.value, total_frames=t.value, frame_format=[k for k, c in _lib.TRAINSET_FORMATS.items() if c == f.value][0],
                    fixations=bool(fl.value & _lib.P3D_TRAINSET_FIXATIONS), bytes=b.value, frames=frames, put=put)

    @staticmethod
    def _u8_frames(a, ndim, what):
        a = np.ascontiguousarray(a)
        if a.dtype != np.uint8 or a.ndim != ndim or (ndim == 4 and a.shape[3] != 3) or a.size == 0:
            raise ValueError("%s are %s %s, expected uint8 %s" % (what, a.dtype, a.shape, "[n, H0, W0, 3]" if ndim == 4 else "[n, H0, W0]"))
        return a

    def trainset_put_frames_u8(self, video, first, bgr):
        """Decoded uint8 frames [n, H0, W0, 3] in cv2's BGR order -> frames first .. first + n - 1 of `video`.  A "u8" set keeps the
        bytes (H0 x W0 must be the grid); an "f32" set keeps dataflow.mapf_frames(bgr, (H, W), mean_rgb), computed on the device."""
        a = self._u8_frames(bgr, 4, "frames")
        check(lib().p3d_trainset_put_frames_u8(self._h, int(video), int(first), a.ctypes.data_as(_lib._u8p), a.shape[0], a.shape[1], a.shape[2]))

    def trainset_put_frames(self, video, first, frames):
        """Normalised float32 frames [n, H, W, 3] -> frames first .. first + n - 1 of `video` ("f32" sets only)."""
        a = np.ascontiguousarray(frames, dtype=np.float32)
        if a.ndim != 4 or a.shape[1:] != self.x_shape[2:] or a.size == 0:
            raise ValueError("frames are %s, the set takes [n, %d, %d, 3]" % (a.shape, self.x_shape[2], self.x_shape[3]))
        check(lib().p3d_trainset_put_frames(self._h, int(video), int(first), fptr(a), len(a)))

    def trainset_put_density_u8(self, video, first, grey):
        """Grey uint8 density maps [n, H0, W0] -> the bytes of dataflow.mapf_density's 8-bit resize to the grid, y = byte / 255."""
        a = self._u8_frames(grey, 3, "density maps")
        check(lib().p3d_trainset_put_density_u8(self._h, int(video), int(first), a.ctypes.data_as(_lib._u8p), a.shape[0], a.shape[1], a.shape[2]))

    def trainset_put_fixations(self, video, first, fix):
        """uint8 fixation maps [n, H, W] on the grid, fixated where the byte is 128 or more (dataflow.fixations_to_grid brings
        full-resolution maps there); the set must have been opened with fixations=True."""
        a = np.ascontiguousarray(fix)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[1:] != self.y_shape[2:] or a.size == 0:
            raise ValueError("fixation maps are %s %s, the set takes uint8 [n, %d, %d]" % (a.dtype, a.shape, self.y_shape[2], self.y_shape[3]))
        check(lib().p3d_trainset_put_fixations(self._h, int(video), int(first), a.ctypes.data_as(_lib._u8p), len(a)))

    @staticmethod
    def _clips(clips):
        c = np.ascontiguousarray(clips, dtype=np.int32)
        if c.ndim != 2 or c.shape[1] != 2:
            raise ValueError("clips is a list of (video, start) pairs")
        return np.ascontiguousarray(c[:, 0]), np.ascontiguousarray(c[:, 1])

    def trainset_stage(self, clips):
        """Cut `batch` clips, (video, start) each, out of the open set into the staged x, y and -- when the set has them -- fixation
        buffers: what upload(x, y, fixations) leaves there for the host-built clips.  Refused with nothing changed when a clip
        leaves its video or holds a frame that was never put."""
        v, st = self._clips(clips)
        check(lib().p3d_trainset_stage(self._h, v.ctypes.data_as(_lib._ip), st.ctypes.data_as(_lib._ip), len(v)))

    def trainset_step(self, clips, dropout=0.5, seed=0):
        """trainset_stage(clips), the augmentation under set_augment, then the train step -> loss: train_step(x, y, dropout, seed,
        fixations) on the host-built clips, bit for bit, without the three uploads."""
        v, st = self._clips(clips)
        loss = C.c_float()
        check(lib().p3d_trainset_step(self._h, v.ctypes.data_as(_lib._ip), st.ctypes.data_as(_lib._ip), len(v), float(dropout), seed, C.byref(loss)))
        return loss.value

    def trainset_forward(self, clips):
        """forward(x, training=False) on the clips' frames, cut on the device; density and fixation maps need not be put."""
        v, st = self._clips(clips)
        pred = np.empty(self.pred_shape, np.float32)
        check(lib().p3d_trainset_forward(self._h, v.ctypes.data_as(_lib._ip), st.ctypes.data_as(_lib._ip), len(v), fptr(pred)))
        return pred

    def trainset_staged(self, fixations=None):
        """The staged inputs read back: (x [B,T,H,W,3], y [B,T,H,W], fix uint8 [B,T,H,W] or None).  fixations: whether to read the
        fixation buffer (default: when the open set has them)."""
        if fixations is None:
            fixations = self.trainset_info()["fixations"]
        x, y = np.empty(self.x_shape, np.float32), np.empty(self.y_shape, np.float32)
        f = np.empty(self.y_shape, np.uint8) if fixations else None
        check(lib().p3d_trainset_get_staged(self._h, fptr(x), fptr(y), f.ctypes.data_as(_lib._u8p) if fixations else None))
        return x, y, f

    def trainset_last_ms(self):
        """HIP-event time of the last trainset_stage / trainset_step / trainset_forward's cut, milliseconds."""
        ms = C.c_double(0.)
        check(lib().p3d_trainset_last_ms(self._h, C.byref(ms)))
        return ms.value

    def upload_fixations(self, fixations):
        """The batch's fixation maps for the losses of _lib.SALIENCY_LOSSES: uint8 [B, T, H, W], fixated where the byte is 128 or
        more (p3d_upload_fixations; dataflow.fixations_to_grid brings full-resolution maps to the grid)."""
        f = np.ascontiguousarray(fixations)
        if f.dtype != np.uint8 or f.shape != self.y_shape:
            raise ValueError("fixations are %s %s, the graph takes uint8 %s" % (f.dtype, f.shape, self.y_shape))
        check(lib().p3d_upload_fixations(self._h, f.ctypes.data_as(C.POINTER(C.c_ubyte))))

    def last_loss_terms(self):
        """The four terms of the last train step or backward under a loss of _lib.SALIENCY_LOSSES, as a trainer logs them:
        {"kld", "cc", "nss", "sim": the mean over this rank's maps where the term is defined (NaN where none is), "counts":
        {name: how many maps those were}} (p3d_last_loss_terms)."""
        sums, counts = (C.c_double * 4)(), (C.c_int64 * 4)()
        check(lib().p3d_last_loss_terms(self._h, sums, counts))
        names = ("kld", "cc", "nss", "sim")
        out = dict((k, sums[i] / counts[i] if counts[i] else float("nan")) for i, k in enumerate(names))
        out["counts"] = dict((k, int(counts[i])) for i, k in enumerate(names))
        return out

    def train_step(self, x, y, dropout=0.5, seed=0, fixations=None):
        """sess.run([train_op, loss], {x, y, dropout, training: True})  (train.py:217-218) -> loss.  fixations: uploaded first
        (upload_fixations)."""
        x, y = self._x(x), self._y(y)
        if fixations is not None:
            self.upload_fixations(fixations)
        loss = C.c_float()
        check(lib().p3d_train_step(self._h, fptr(x), fptr(y), float(dropout), seed, C.byref(loss)))
        return loss.value

    def backward(self, x, y, dropout=0.0, seed=0, fixations=None):
        """Forward + loss + gradients without the update -> (loss, pred).  fixations: uploaded first (upload_fixations)."""
        x, y = self._x(x), self._y(y)
        if fixations is not None:
            self.upload_fixations(fixations)
        loss = C.c_float()
        pred = np.empty(self.pred_shape, np.float32)
        check(lib().p3d_backward(self._h, fptr(x), fptr(y), float(dropout), seed, C.byref(loss), fptr(pred)))
        return loss.value, pred

    def evaluate(self, x, density, fixation, size=(1080, 960), jitter=True, n_rep=100, step_size=0.1, rng=None, shuffled=None):
        """The per-batch body of test.py (test.py:160-176) -> [B, 5] float64: CC, SIM, AUC_Judd, AUC_Borji, NSS of the last
        frame of every clip, scored at the fixation maps' resolution.  One plain batched forward with training False (:160:
        the backbone BatchNorm couples the clips of a batch, as in the reference), then one device pass that resizes the
        prediction (cv2.resize(prediction, (960, 1080)), :170) and the density map (dataflow.py:236-238) and computes the
        five metrics; only the five numbers per clip come back.
        density: uint8 [B, Hd, Wd] or [B, T, Hd, Wd]; fixation: uint8 [B, H, W] or [B, T, H, W] with (H, W) == size; the last
        frame is used (:167-169).  numpy's stream (`rng`, default np.random, as utils/metrics.py draws) is consumed per clip
        in the reference's order: AUC_Judd's random.rand(H, W) (jitter=True, :64-65), then AUC_Borji's
        random.randint(0, H*W, [n_fix, n_rep]) (:139); a clip without fixation draws nothing (:56-59, :122-124).
        Stage times of the call are left in `last_eval_ms` (forward, draws, h2d, device; milliseconds).
        shuffled (default None: nothing changes): dict(others=int [B, M] slots of the open fixation pool, rng=a RandomState of its
        own, n_rep=100, step_size=0.1) adds shuffled AUC of the clean scored map in the same device pass: the union is taken
        (shuffled_begin; skipped when the dict carries the n_other a caller's own shuffled_begin returned), metrics.shuffled_draws
        draws from `rng`, and last_eval_shuffled() returns the result.  The five columns are the same bits either way."""
        import time
        H, W = (size, size) if np.isscalar(size) else tuple(size)
        B = self.x_shape[0]
        dens = np.asarray(density)
        fix = np.asarray(fixation)
        if dens.dtype != np.uint8 or fix.dtype != np.uint8:
            raise ValueError("density and fixation maps are uint8 images (cv2.IMREAD_GRAYSCALE)")
        dens = np.ascontiguousarray(dens[:, -1] if dens.ndim == 4 else dens)
        fix = np.ascontiguousarray(fix[:, -1] if fix.ndim == 4 else fix)
        if dens.ndim != 3 or dens.shape[0] != B or fix.ndim != 3 or fix.shape[0] != B:
            raise ValueError("expected %d density / fixation maps, [B, H, W] or [B, T, H, W]" % B)
        if fix.shape[1:] != (H, W):
            raise ValueError("fixation maps are %s, not %s: the reference would resize the prediction to them through skimage, "
                             "which this library does not reproduce" % (fix.shape[1:], (H, W)))
        t0 = time.perf_counter()
        self.upload(x, None)
        self.forward_device(training=False)
        self.synchronize()
        t1 = time.perf_counter()
        n_fix, jit, idx = eval_draws(fix, bool(jitter), n_rep, rng)
        if shuffled is not None:
            from .metrics import shuffled_draws
            n_other = shuffled["n_other"] if shuffled.get("n_other") is not None else self.shuffled_begin(shuffled["others"])
            s_rep = int(shuffled.get("n_rep", 100))
            if "ranks" in shuffled:             # (tests of the refusals: ranks of the caller's, nothing drawn)
                ranks, n_rows = (np.ascontiguousarray(v, dtype=np.int32) for v in (shuffled["ranks"], shuffled["n_rows"]))
            else:
                ranks, n_rows = shuffled_draws(n_fix, n_other, s_rep, shuffled.get("rng"))
            check(lib().p3d_eval_shuffled_draws(self._h, ranks.ctypes.data_as(_lib._ip), n_rows.ctypes.data_as(_lib._ip), s_rep,
                                                float(shuffled.get("step_size", 0.1))))
            self._shuffled_rep = s_rep
        t2 = time.perf_counter()
        out = np.empty((B, 5), np.float64)
        ms = (C.c_double * 2)()
        u8 = C.POINTER(C.c_ubyte)
        check(lib().p3d_eval_last_frames(self._h, dens.ctypes.data_as(u8), dens.shape[1], dens.shape[2], fix.ctypes.data_as(u8),
                                         H, W, jit.ctypes.data_as(_lib._dp) if jit is not None else None,
                                         idx.ctypes.data_as(_lib._ip), n_fix.ctypes.data_as(_lib._ip), int(n_rep), float(step_size),
                                         out.ctypes.data_as(_lib._dp), ms))
        self.last_eval_ms = dict(forward=(t1 - t0) * 1e3, draws=(t2 - t1) * 1e3, h2d=ms[0], device=ms[1])
        return out

    def set_adam(self, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8):
        check(lib().p3d_set_adam(self._h, lr, beta1, beta2, eps))
        self._betas = (beta1, beta2)

    # ---- optimiser (p3d_set_optimizer) and its state -------------------------------------------------
    def set_optimizer(self, name="adam", lr=1e-4, momentum=0.9, use_nesterov=False):
        """The train step's optimiser: "adam" (tf.train.AdamOptimizer; beta1, beta2, eps stay as set_adam left them),
        "momentum" (tf.train.MomentumOptimizer(lr, momentum, use_nesterov)) or "sgd" (tf.train.GradientDescentOptimizer(lr)).
        Switching kind starts a fresh optimiser (zero slots, step 0); the same kind with new values keeps its state."""
        if name not in _lib.OPTIMIZERS:
            raise ValueError("optimizer %r: have %s" % (name, sorted(_lib.OPTIMIZERS)))
        check(lib().p3d_set_optimizer(self._h, _lib.OPTIMIZERS[name], float(lr), float(momentum), 1 if use_nesterov else 0))
        self._opt = name

    def optimizer_step(self):
        """Completed optimiser steps."""
        t = C.c_int64()
        check(lib().p3d_get_optimizer_step(self._h, C.byref(t)))
        return t.value

    def _slot_names(self):
        return slot_names(self.variables(), self._opt)

    def get_slot(self, name, slot):
        shape = dict((n, s) for n, s, _ in self.variables())[name]
        a = np.empty(shape, np.float32)
        check(lib().p3d_get_slot(self._h, name.encode(), int(slot), fptr(a), a.size))
        return a

    def set_slot(self, name, slot, value):
        a = np.ascontiguousarray(value, dtype=np.float32)
        check(lib().p3d_set_slot(self._h, name.encode(), int(slot), fptr(a), a.size))

    def optimizer_state(self):
        """{TF name: array} of the optimiser's state, as a default tf.train.Saver stores it: <var>/Adam and <var>/Adam_1 (m, v)
        with the float32 scalars beta1_power and beta2_power for Adam -- TF keeps b^(t+1) after t completed steps (the
        variables start at b and are multiplied after each step) --, <var>/Momentum for Momentum, nothing for SGD."""
        out = dict((k, self.get_slot(n, i)) for k, (n, i) in self._slot_names().items())
        if self._opt == "adam":
            t = self.optimizer_step()
            for key, b in zip(("beta1_power", "beta2_power"), self._betas):
                out[key] = np.array(np.float64(np.float32(b)) ** (t + 1), np.float32)
        return out

    def _parse_optimizer_state(self, d):
        slots = self._slot_names()
        missing = sorted(k for k in slots if k not in d)
        if self._opt == "adam":
            missing += [k for k in ("beta1_power", "beta2_power") if k not in d]
        if missing:
            raise KeyError("checkpoint lacks %d %s slots, e.g. %s" % (len(missing), self._opt, missing[:3]))
        t = adam_step_from_powers(d["beta1_power"], d["beta2_power"], *self._betas) if self._opt == "adam" else None
        return slots, t

    def load_optimizer_state(self, d):
        """Set the current optimiser's slots from {TF name: array} (optimizer_state()'s form; extra names are ignored).  For
        Adam the completed steps t are the integer nearest to log(beta2_power) / log(beta2) - 1; a beta1_power that does not
        fit that t (relative 1e-3, beyond float32's smallest normal) refuses the checkpoint: TF's running float32 product
        drifts, so the powers are not compared bit for bit."""
        slots, t = self._parse_optimizer_state(d)
        for k, (n, i) in slots.items():
            self.set_slot(n, i, d[k])
        if t is not None:
            check(lib().p3d_set_optimizer_step(self._h, int(t)))

    def activation(self, name):
        shape = (C.c_int64 * 5)()
        check(lib().p3d_activation_info(self._h, name.encode(), shape))
        a = np.empty(tuple(shape), np.float32)
        check(lib().p3d_get_activation(self._h, name.encode(), fptr(a), a.size))
        return a

    # ---- device-resident stepping (bench) ------------------------------------------------------
    def upload(self, x, y, fixations=None):
        check(lib().p3d_upload_inputs(self._h, fptr(self._x(x)), fptr(self._y(y)) if y is not None else None))
        if fixations is not None:
            self.upload_fixations(fixations)

    def bucket_audit(self, bucket_floats, dropout=0.0, seed=0, cap=4096):
        """Test hook for the bucketed gradient hand-over of data-parallel training (include/p3d_hip.h,
        p3d_debug_bucket_audit): ([(lo, hi, after_op)], n_train, stale)."""
        lo = (C.c_int64 * cap)(); hi = (C.c_int64 * cap)(); op = (C.c_int32 * cap)()
        n_train = C.c_int64(); stale = C.c_int64()
        n = lib().p3d_debug_bucket_audit(self._h, float(dropout), seed, int(bucket_floats), lo, hi, op, cap, C.byref(n_train),
                                         C.byref(stale))
        if n < 0:
            check(n)
        return [(lo[i], hi[i], op[i]) for i in range(min(n, cap))], n_train.value, stale.value

    def train_step_device(self, dropout=0.0, seed=0):
        check(lib().p3d_train_step_device(self._h, float(dropout), seed))

    def forward_device(self, training=False, dropout=0.0, seed=0):
        check(lib().p3d_forward_device(self._h, int(bool(training)), float(dropout), seed))

    def last_loss(self):
        loss = C.c_float()
        check(lib().p3d_last_loss(self._h, C.byref(loss)))
        return loss.value

    def synchronize(self):
        check(lib().p3d_synchronize(self._h))

    def profile_step(self, dropout=0.0, seed=0):
        cap = 16384
        buf = (P3dOpTime * cap)()
        n = lib().p3d_profile_step(self._h, float(dropout), seed, buf, cap)
        if n < 0:
            raise P3dError(lib().p3d_last_error().decode())
        return [dict(name=r.name.decode(), kernel=r.kernel.decode(), ms=r.ms, flops=r.flops, bytes=r.bytes,
                     phase=r.phase) for r in buf[:min(n, cap)]]

    # ---- data parallel -----------------------------------------------------------------------------
    @staticmethod
    def device_count():
        """GPUs visible to this process (-1: the runtime could not say)."""
        return lib().p3d_device_count()

    @staticmethod
    def comm_unique_id():
        buf = C.create_string_buffer(_lib.P3D_COMM_ID_BYTES)
        check(lib().p3d_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, id_bytes):
        buf = C.create_string_buffer(bytes(id_bytes), _lib.P3D_COMM_ID_BYTES)
        check(lib().p3d_comm_init(self._h, buf))

    def comm_info(self):
        """(ranks, rank, device) as RCCL reports them for this handle's communicator; ranks == 0: no communicator."""
        n, r, d = C.c_int(0), C.c_int(-1), C.c_int(-1)
        check(lib().p3d_comm_info(self._h, C.byref(n), C.byref(r), C.byref(d)))
        return n.value, r.value, d.value
