"""The TensorFlow ops the reference's P3D path is made of, as eager numpy-in / numpy-out calls
into the HIP kernels (argument order and meaning follow tf.nn.* / tf.layers.*)."""
import ctypes as C

import numpy as np

from ._lib import LOSSES, OPTIMIZERS, check, fptr, lib


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _shape5(s):
    return (C.c_int64 * 5)(*[int(v) for v in s])


def _i3(s):
    return (C.c_int * 3)(*[int(v) for v in s])


def _same_out(size, s):
    return -(-size // s)


def _strides3(strides):
    strides = list(strides)
    if len(strides) == 5:
        if strides[0] != 1 or strides[4] != 1:
            raise ValueError("strides must be [1, sd, sh, sw, 1]")
        strides = strides[1:4]
    return strides


def conv3d(x, filter, strides, padding="SAME", bias=None, device=0):
    """tf.nn.conv3d(x, filter, strides, 'SAME') (+ tf.nn.bias_add)."""
    if padding.upper() != "SAME":
        raise ValueError("only SAME padding is on the P3D path")
    x, w = _f32(x), _f32(filter)
    s = _strides3(strides)
    if w.shape[3] != x.shape[4]:
        raise ValueError("filter in-channels %d != input channels %d" % (w.shape[3], x.shape[4]))
    y = np.empty((x.shape[0],) + tuple(_same_out(x.shape[1 + i], s[i]) for i in range(3)) + (w.shape[4],), np.float32)
    b = _f32(bias) if bias is not None else None
    check(lib().p3d_op_conv3d(device, fptr(x), _shape5(x.shape), fptr(w), _shape5(w.shape), _i3(s), fptr(b), fptr(y)))
    return y


def conv3d_backprop_input(input_sizes, filter, out_backprop, strides, device=0):
    """tf.nn.conv3d_backprop_input_v2."""
    w, dy = _f32(filter), _f32(out_backprop)
    s = _strides3(strides)
    dx = np.empty(tuple(input_sizes), np.float32)
    check(lib().p3d_op_conv3d_backprop_input(device, fptr(dy), fptr(w), _shape5(w.shape), _i3(s), _shape5(input_sizes), fptr(dx)))
    return dx


def conv3d_backprop_filter(input, filter_sizes, out_backprop, strides, with_bias=False, device=0):
    """tf.nn.conv3d_backprop_filter_v2 (optionally also the bias_add gradient)."""
    x, dy = _f32(input), _f32(out_backprop)
    s = _strides3(strides)
    dw = np.empty(tuple(filter_sizes), np.float32)
    db = np.empty((filter_sizes[4],), np.float32) if with_bias else None
    check(lib().p3d_op_conv3d_backprop_filter(device, fptr(x), _shape5(x.shape), fptr(dy), _shape5(filter_sizes), _i3(s),
                                             fptr(dw), fptr(db)))
    return (dw, db) if with_bias else dw


def conv3d_transpose(x, kernel, strides, bias=None, device=0):
    """tf.layers.conv3d_transpose(x, filters, k, strides, 'same'); kernel is [kd,kh,kw,Cout,Cin]."""
    x, k = _f32(x), _f32(kernel)
    s = _strides3(strides)
    y = np.empty((x.shape[0], x.shape[1] * s[0], x.shape[2] * s[1], x.shape[3] * s[2], k.shape[3]), np.float32)
    b = _f32(bias) if bias is not None else None
    check(lib().p3d_op_conv3d_transpose(device, fptr(x), _shape5(x.shape), fptr(k), _shape5(k.shape), _i3(s), fptr(b), fptr(y)))
    return y


def conv_bn_stats(x, filter, strides, bias=None, transpose=False, filter2=None, moving=None, device=0):
    """Test hook: a conv (transpose: tf.layers.conv3d_transpose, kernel [kd,kh,kw,Cout,Cin]) followed by the statistics step of
    tf.layers.batch_normalization in training, as the network runs it (the conv's statistics epilogue, then the finalize).
    filter2: a sibling conv on the same input, sent with the first as the network sends a pair.  moving: [pairs, 2, C] moving
    (mean, variance) before the update (default zeros / ones).  Returns (ys, mean, invstd, moving after, nparts, kernel),
    ys / mean / invstd / nparts with one entry per conv."""
    x, w = _f32(x), _f32(filter)
    s = _strides3(strides)
    pairs = 2 if filter2 is not None else 1
    if transpose:
        C_ = w.shape[3]
        yshape = (x.shape[0], x.shape[1] * s[0], x.shape[2] * s[1], x.shape[3] * s[2], C_)
    else:
        C_ = w.shape[4]
        yshape = (x.shape[0],) + tuple(_same_out(x.shape[1 + i], s[i]) for i in range(3)) + (C_,)
    if moving is None:
        moving = np.stack([np.stack([np.zeros(C_), np.ones(C_)])] * pairs)
    mv = np.array(moving, dtype=np.float32).reshape(pairs, 2, C_).copy()
    ys = [np.empty(yshape, np.float32) for _ in range(pairs)]
    stats = np.empty((pairs, 4, C_), np.float32)
    nparts = (C.c_int * 2)()
    kernel = C.c_char_p()
    w2 = _f32(filter2) if filter2 is not None else None
    b = _f32(bias) if bias is not None else None
    check(lib().p3d_debug_conv_bn_stats(device, fptr(x), _shape5(x.shape), fptr(w), fptr(w2), _shape5(w.shape), _i3(s), fptr(b),
                                        1 if transpose else 0, fptr(mv), fptr(ys[0]), fptr(ys[1]) if pairs == 2 else None,
                                        fptr(stats), nparts, C.byref(kernel)))
    return ys, stats[:, 2], stats[:, 3], mv, [nparts[q] for q in range(pairs)], kernel.value.decode()


def bn_pass(mode, y1, y2, params, moving, dz, batch=(1, 1), update_moving=1, acc2=None, path=0, device=0, C_=None,
            offset=(0, 0, 0), drop_rate=0.0, seed=0, seed_dev=False, z=None, dy1=None, dy2=None):
    """Test hook: one BatchNorm normalise / ReLU / add pass of the network (mode 0-4, see include/p3d_hip.h) forward and
    backward on [M, C] arrays.  params [bns, 2, C] = gamma, beta; moving [bns, 2, C] moving (mean, variance) before.
    acc2: the gradient of y2 to add to (None: overwrite).  path 0 = the network's rule, 1 small, 2 fold-apply, 3 finalize +
    apply.  Returns (z, dy1, dy2, grads [bns, 2, C], moving after, (path taken, forward partials, backward partials)).

    C_ (default: dense operands, as above): the operands are C_-channel slices of the wide buffers y1 [M, ld1], y2 [M, ld2] and
    dz [M, ldz] at the column offsets `offset` (of y1 / dy1, of y2 / dy2, of z / dz); z, dy1 and dy2 are then what the wide
    output buffers hold before the pass (dy2 inside its slice: the gradient to add to when acc2 is not None, whose value is
    otherwise unused), and the wide buffers are returned.  drop_rate > 0: the pass drops out with the kernels' mask of `seed`,
    passed as an argument or (seed_dev) read from device memory."""
    y1 = _f32(y1)
    bns = 2 if mode in (2, 3) else 1
    y2 = _f32(y2) if mode != 0 else None
    dz = _f32(dz)
    if C_ is None:
        M, C_ = y1.shape
        z, dy1 = np.empty((M, C_), np.float32), np.empty((M, C_), np.float32)
        dy2 = (_f32(acc2).copy() if acc2 is not None else np.empty((M, C_), np.float32)) if mode != 0 else None
    else:
        M, C_ = y1.shape[0], int(C_)
        if z is None or dy1 is None or (mode != 0 and dy2 is None):
            raise ValueError("bn_pass: sliced operands come with the z, dy1 and dy2 buffers")
        z, dy1 = _f32(z).copy(), _f32(dy1).copy()
        dy2 = _f32(dy2).copy() if mode != 0 else None
        if z.shape != dz.shape or dy1.shape != y1.shape or (mode != 0 and dy2.shape != y2.shape):
            raise ValueError("bn_pass: z, dy1, dy2 have the shapes of dz, y1, y2")
    if dz.shape[0] != M or (mode != 0 and y2.shape[0] != M):
        raise ValueError("bn_pass: every operand has M rows")
    prm = _f32(np.asarray(params).reshape(bns, 2, C_))
    mv = np.array(moving, dtype=np.float32).reshape(bns, 2, C_).copy()
    grads = np.empty((bns, 2, C_), np.float32)
    info = (C.c_int * 3)()
    ld2 = y2.shape[1] if mode != 0 else C_
    check(lib().p3d_debug_bn_pass(device, mode, M, C_, fptr(y1), y1.shape[1], int(offset[0]), fptr(y2), ld2, int(offset[1]),
                                  fptr(prm), int(batch[0]), int(batch[1]), int(update_moving), fptr(dz),
                                  1 if acc2 is not None else 0, float(drop_rate), int(seed), 1 if seed_dev else 0, path, fptr(z),
                                  z.shape[1], int(offset[2]), fptr(dy1), fptr(dy2), fptr(grads), fptr(mv), info))
    return z, dy1, dy2, grads, mv, tuple(info)


def _strided(a, ld, fill):
    """[rows, C] -> [rows, ld] float32 with `fill` in the columns past C."""
    a = _f32(a)
    out = np.full((a.shape[0], ld), fill, np.float32)
    out[:, :a.shape[1]] = a
    return out


def gn_pass(mode, y1, y2, params, dz, G, eps=1e-5, cs=None, ss=None, acc2=None, grads=None, drop_rate=0.0, seed=0, path=0,
            ld=(None, None, None), pad=np.nan, device=0):
    """Test hook: one GroupNorm normalise / ReLU / add pass of the GN network (mode 0-6, see include/p3d_hip.h) forward and
    backward (mode 2: forward only) on [N, R, C] arrays with G groups.  params [gns, 2, C] = gamma, beta; cs [N, C], ss [N, R]
    for mode 6.  acc2: the gradient of y2 to add to (None: overwrite).  grads: [gns, 2, C] held by the parameter gradients
    before the pass (default NaN: they must be stored).  ld = (ld of y1 / dy1, of y2 / dy2, of z / dz), None for C: the
    operands are then stored with rows of ld floats, the columns past C filled with `pad`.  path 0 = the network's rule, 1 small,
    2 statistics / finalize / apply.  Returns (z, dy1, dy2, grads, tables [gns, 4, N, C] = scale, shift, mean, invstd,
    path taken, pads) -- z, dy1, dy2 [N, R, C] (None where the mode has none); pads = what z, dy1, dy2 held past column C."""
    y1 = _f32(y1)
    N, R, C_ = y1.shape
    M = N * R
    gns = 2 if mode in (2, 3) else 1
    has2, bwd = mode not in (0, 5), mode != 2
    d2 = mode in (1, 3, 4, 6)
    l1, l2, lz = [C_ if v is None else int(v) for v in ld]
    y1s = _strided(y1.reshape(M, C_), l1, pad)
    y2s = _strided(_f32(y2).reshape(M, C_), l2, pad) if has2 else None
    dzs = _strided(_f32(dz).reshape(M, C_), lz, pad) if bwd else None
    zs = np.full((M, lz), pad, np.float32)
    g1s = np.full((M, l1), pad, np.float32)
    if d2:
        g2s = _strided(_f32(acc2).reshape(M, C_), l2, pad) if acc2 is not None else np.full((M, l2), pad, np.float32)
    else:
        g2s = None
    prm = _f32(np.asarray(params).reshape(gns, 2, C_))
    grd = np.full((gns, 2, C_), np.nan, np.float32) if grads is None else _f32(np.asarray(grads).reshape(gns, 2, C_)).copy()
    tables = np.empty((gns, 4, N, C_), np.float32)
    csd = _f32(np.asarray(cs).reshape(N, C_)) if mode == 6 else None
    ssd = _f32(np.asarray(ss).reshape(M)) if mode == 6 else None
    info = (C.c_int * 1)()
    check(lib().p3d_debug_gn_pass(device, mode, N, R, C_, int(G), float(eps), fptr(y1s), l1, fptr(y2s), l2, lz, fptr(prm),
                                  fptr(csd), fptr(ssd), fptr(dzs), 1 if acc2 is not None else 0, float(drop_rate), int(seed),
                                  path, fptr(zs), fptr(g1s), fptr(g2s), fptr(grd), fptr(tables), info))
    z = zs[:, :C_].reshape(N, R, C_).copy()
    dy1 = g1s[:, :C_].reshape(N, R, C_).copy() if bwd else None
    dy2 = g2s[:, :C_].reshape(N, R, C_).copy() if (bwd and d2) else None
    pads = (zs[:, C_:], g1s[:, C_:], g2s[:, C_:] if g2s is not None else None)
    return z, dy1, dy2, (grd if bwd else None), tables, info[0], pads


def cbam(x, k0, b0, k1, b1, k7, dout, chunks=0, dx=None, pgrads=None, ld=None, pad=np.nan, device=0):
    """Test hook: CBAM (utils/network.py:198-274) forward and backward on x [N, D, H, W, C] as the network runs it.  k0 [C, C/8],
    b0 [C/8], k1 [C/8, C], b1 [C], k7 [7, 7, 7, 2, 1]; dout: gradient of the output.  chunks: row chunks per sample (0: the
    network's rule).  dx: the gradient of x to add to (None: overwrite); pgrads: (dk0, db0, dk1, db1, dk7) to add to (None:
    zeros).  ld: row stride of x and dx (None: C; the columns past C hold `pad`).  Returns (cs [N, C], sp [N, D, H, W, 2],
    ss [N, D, H, W], dx, (dk0, db0, dk1, db1, dk7), chunks used, what dx held past column C)."""
    x = _f32(x)
    N, D, H, W, C_ = x.shape
    Ch = C_ // 8
    M = N * D * H * W
    l = C_ if ld is None else int(ld)
    xs = _strided(x.reshape(M, C_), l, pad)
    dxs = _strided(_f32(dx).reshape(M, C_), l, pad) if dx is not None else np.full((M, l), pad, np.float32)
    shapes = [(C_, Ch), (Ch,), (Ch, C_), (C_,), (7, 7, 7, 2, 1)]
    if pgrads is None:
        pgrads = [np.zeros(s, np.float32) for s in shapes]
    pg = np.concatenate([_f32(np.asarray(g).reshape(s)).ravel() for g, s in zip(pgrads, shapes)])
    cs, sp, ss = np.empty((N, C_), np.float32), np.empty((M, 2), np.float32), np.empty((M,), np.float32)
    info = (C.c_int * 1)()
    check(lib().p3d_debug_cbam(device, N, D, H, W, C_, fptr(xs), l, fptr(_f32(k0)), fptr(_f32(b0)), fptr(_f32(k1)), fptr(_f32(b1)),
                               fptr(_f32(k7)), int(chunks), fptr(_f32(dout)), 1 if dx is not None else 0, fptr(cs), fptr(sp),
                               fptr(ss), fptr(dxs), fptr(pg), info))
    out, o = [], 0
    for s in shapes:
        n = int(np.prod(s))
        out.append(pg[o:o + n].reshape(s))
        o += n
    return (cs, sp.reshape(N, D, H, W, 2), ss.reshape(N, D, H, W), dxs[:, :C_].reshape(x.shape).copy(), tuple(out), info[0],
            dxs[:, C_:])


def _embed(a, ld, offset, fill):
    """[rows, C] -> [rows, ld] float32 holding `a` in columns offset .. offset + C and `fill` in every other column."""
    a = _f32(a)
    out = np.full((a.shape[0], int(ld)), fill, np.float32)
    out[:, offset:offset + a.shape[1]] = a
    return out


def _outside(buf, C_, offset):
    """The columns of [rows, ld] `buf` that are not in the slice offset .. offset + C (left of it, then right of it)."""
    return np.concatenate([buf[:, :offset], buf[:, offset + C_:]], axis=1)


CONV_KINDS = {"forward": 0, "input_grad": 1, "transpose": 2}


def conv_launch(kind, inp, filter, strides, input_sizes=None, bias=None, accum=False, f16=False, ld=(None, None), offset=(0, 0),
                pad=np.nan, prior=np.nan, device=0):
    """Test hook: one conv of the network in the launch form the train step uses (p3d_debug_conv_launch).  kind "forward"
    (inp = x), "input_grad" (inp = dy, input_sizes = shape of x) or "transpose" (tf.layers.conv3d_transpose, filter
    [kd,kh,kw,Cout,Cin]).  ld = (row length of the gathered operand, of the output), None for its channel count; offset = the
    channel offsets of the two slices; every column outside a slice holds `pad`.  prior: what the output slice holds before the
    launch (scalar or array of the output's shape); accum: the launch adds to it.  f16: the fp16 option (1x1x1 only).  Returns
    (the output slice, everything outside it [rows, ld - C], the kernel names joined with ';'); conv_launch.last_splits = the
    (smallest, largest) K-slice count of the launches' plans."""
    x, w = _f32(inp), _f32(filter)
    s = _strides3(strides)
    kd = CONV_KINDS[kind]
    if kd == 0:
        xshape = x.shape
        oshape = (x.shape[0],) + tuple(_same_out(x.shape[1 + i], s[i]) for i in range(3)) + (w.shape[4],)
    elif kd == 1:
        xshape = tuple(int(v) for v in input_sizes)
        oshape = xshape
    else:
        xshape = x.shape
        oshape = (x.shape[0], x.shape[1] * s[0], x.shape[2] * s[1], x.shape[3] * s[2], w.shape[3])
    ci, co = x.shape[4], oshape[4]
    l_in, l_out = (c if v is None else int(v) for v, c in zip(ld, (ci, co)))
    o_in, o_out = (int(v) for v in offset)
    xin = _embed(x.reshape(-1, ci), l_in, o_in, pad)
    rows_out = int(np.prod(oshape[:4]))
    pr = np.broadcast_to(np.asarray(prior, np.float32), oshape).reshape(rows_out, co)
    out = _embed(pr, l_out, o_out, pad)
    b = _f32(bias) if bias is not None else None
    names = C.create_string_buffer(16384)
    splits = (C.c_int * 2)()
    check(lib().p3d_debug_conv_launch(device, kd, fptr(xin), l_in, o_in, _shape5(xshape), fptr(w), _shape5(w.shape), _i3(s), fptr(b),
                                      1 if accum else 0, 1 if f16 else 0, fptr(out), l_out, o_out, names, len(names), splits))
    conv_launch.last_splits = (splits[0], splits[1])
    return out[:, o_out:o_out + co].reshape(oshape).copy(), _outside(out, co, o_out), names.value.decode()


def wgrad_group(problems, polite=False, greedy=False, pad=np.nan, device=0):
    """Test hook: up to 6 filter gradients as ONE launch, the way the train step's queue sends them (p3d_debug_wgrad_group).
    Each problem is a dict: x, dy, filter_sizes, strides, and optionally ld = (row length of x, of dy), offset = (channel offset
    of x, of dy), dw / dbias = what the gradients hold before (dw default zeros; dbias None: no bias gradient), transpose (a
    transposed conv's problem: x its input, dy the gradient of its output, filter_sizes [kd,kh,kw,Cout,Cin]).  Columns outside the
    slices hold `pad`.  Returns ([(dw, dbias or None), ...], kernel name, cuts per problem (0: dropped), (slab stride, tile rows,
    tile columns))."""
    n = len(problems)
    xs, dys, dws, dbs, keep = [], [], [], [], []
    ldx, offx, lddy, offdy, tr = [], [], [], [], []
    xsh, wsh, st = [], [], []
    for pr in problems:
        x, dy = _f32(pr["x"]), _f32(pr["dy"])
        fs = tuple(int(v) for v in pr["filter_sizes"])
        l = pr.get("ld", (None, None))
        o = pr.get("offset", (0, 0))
        lx, ly = (c if v is None else int(v) for v, c in zip(l, (x.shape[4], dy.shape[4])))
        xs.append(_embed(x.reshape(-1, x.shape[4]), lx, int(o[0]), pad))
        dys.append(_embed(dy.reshape(-1, dy.shape[4]), ly, int(o[1]), pad))
        dws.append(np.zeros(fs, np.float32) if pr.get("dw") is None else _f32(np.asarray(pr["dw"]).reshape(fs)).copy())
        dbs.append(None if pr.get("dbias") is None else _f32(np.asarray(pr["dbias"]).reshape(fs[3] if pr.get("transpose") else fs[4])).copy())
        ldx.append(lx); offx.append(int(o[0])); lddy.append(ly); offdy.append(int(o[1])); tr.append(1 if pr.get("transpose") else 0)
        xsh += [int(v) for v in x.shape]
        wsh += list(fs)
        st += [int(v) for v in _strides3(pr["strides"])]
    fpp = type(fptr(dws[0]))
    arr = lambda v: (fpp * n)(*[fptr(a) for a in v])
    ints = lambda v: (C.c_int * len(v))(*v)
    name = C.create_string_buffer(256)
    cuts, info = (C.c_int * n)(), (C.c_int * 3)()
    check(lib().p3d_debug_wgrad_group(device, n, arr(xs), ints(ldx), ints(offx), (C.c_int64 * len(xsh))(*xsh), arr(dys), ints(lddy),
                                      ints(offdy), (C.c_int64 * len(wsh))(*wsh), ints(st), ints(tr), arr(dws), arr(dbs),
                                      1 if polite else 0, 1 if greedy else 0, name, len(name), cuts, info))
    return list(zip(dws, dbs)), name.value.decode(), list(cuts), tuple(info)


def _own(a, shape=None):
    """A private float32 copy of an in / out array (None stays None)."""
    if a is None:
        return None
    a = np.array(a, dtype=np.float32, order="C", copy=True)
    return a if shape is None else a.reshape(shape)


def fused_conv(kind, input_sizes, filter, strides, out, ld_out=None, off_out=0, bias=None, f16=False, src=(), g=None, ld_g=None,
               off_g=0, grad=None, gates=(), raw_store=False, accum=False, device=0):
    """Test hook: one fused-BatchNorm conv launch (p3d_debug_fused_conv), built by the builders of the graph's conv op.
    kind "forward": src = one (RELU1) or two (RELU2) dicts {y [rows, ld], off, and either scale / shift (published) or gamma,
    beta, partials [nparts, C, 2], rows, publish, update_moving, moving_mean, moving_var}; scale, shift, mean, invstd are what
    the published arrays hold before.  kind "input_grad": g [rows, ld_g] the gradient of the conv's output; grad = dict {y
    [rows, ld], off, coef [3, Cout] and either nothing more (published) or gamma, mean, invstd, partials [nparts, Cout, 2], rows,
    publish, dgamma, dbeta}; gates = up to two dicts {y [rows, ld], off_y, scale, shift, mean, invstd, out [rows, ld_out], off_out,
    part [part_rows, Cin, 2]}.  out [rows, ld_out]: what the output / raw-result buffer holds before.  Two sources that pass the
    same array object as y share one device buffer.  Nothing passed in is modified; returns a dict: out, kernels, splits, src
    (list of dicts scale, shift, mean, invstd, moving_mean, moving_var), grad (coef, dgamma, dbeta), gates (list of out, part),
    gpart_rows."""
    from ._lib import P3dFusedConv
    kd = CONV_KINDS[kind]
    if kd > 1:
        raise ValueError("fused_conv: forward or input_grad")
    w = _f32(filter)
    a = P3dFusedConv()
    keep = [w]
    a.kind = kd
    a.xshape = _shape5(input_sizes)
    a.wshape = _shape5(w.shape)
    a.stride = _i3(_strides3(strides))
    a.w = fptr(w)
    b = _f32(bias) if bias is not None else None
    keep.append(b)
    a.bias = fptr(b)
    a.f16 = 1 if f16 else 0
    res = {"src": [], "grad": None, "gates": []}
    o = _own(out)
    a.out, a.ld_out, a.off_out = fptr(o), int(o.shape[1] if ld_out is None else ld_out), int(off_out)
    ro = lambda v: None if v is None else _f32(v)
    if kd == 0:
        a.at = len(src)
        shared = {}
        for q, sd in enumerate(src):
            f = a.src[q]
            y = shared.setdefault(id(sd["y"]), _f32(sd["y"]))
            arrs = {k: ro(sd.get(k)) for k in ("gamma", "beta", "partials")}
            outs = {k: _own(sd.get(k)) for k in ("scale", "shift", "mean", "invstd", "moving_mean", "moving_var")}
            keep += [y, arrs, outs]
            f.y, f.ld, f.off = fptr(y), y.shape[1], int(sd.get("off", 0))
            f.gamma, f.beta, f.partials = fptr(arrs["gamma"]), fptr(arrs["beta"]), fptr(arrs["partials"])
            f.nparts = 0 if arrs["partials"] is None else arrs["partials"].shape[0]
            f.rows = int(sd.get("rows", 0))
            f.publish, f.update_moving = (1 if sd.get("publish") else 0), (1 if sd.get("update_moving") else 0)
            f.scale, f.shift, f.mean, f.invstd = (fptr(outs[k]) for k in ("scale", "shift", "mean", "invstd"))
            f.moving_mean, f.moving_var = fptr(outs["moving_mean"]), fptr(outs["moving_var"])
            res["src"].append(outs)
    else:
        gg = _f32(g)
        keep.append(gg)
        a.g, a.ld_g, a.off_g = fptr(gg), int(gg.shape[1] if ld_g is None else ld_g), int(off_g)
        if grad is not None:
            a.grad = 1
            f = a.gbn
            y = _f32(grad["y"])
            arrs = {k: ro(grad.get(k)) for k in ("gamma", "mean", "invstd", "partials")}
            outs = {k: _own(grad.get(k)) for k in ("coef", "dgamma", "dbeta")}
            keep += [y, arrs, outs]
            f.y, f.ld, f.off = fptr(y), y.shape[1], int(grad.get("off", 0))
            f.gamma, f.mean, f.invstd, f.partials = (fptr(arrs[k]) for k in ("gamma", "mean", "invstd", "partials"))
            f.nparts = 0 if arrs["partials"] is None else arrs["partials"].shape[0]
            f.rows = int(grad.get("rows", 0))
            f.publish = 1 if grad.get("publish") else 0
            f.coef, f.dgamma, f.dbeta = fptr(outs["coef"]), fptr(outs["dgamma"]), fptr(outs["dbeta"])
            res["grad"] = outs
        a.ngate = len(gates)
        for q, gd in enumerate(gates):
            f = a.gate[q]
            y = _f32(gd["y"])
            tabs = {k: _f32(gd[k]) for k in ("scale", "shift", "mean", "invstd")}
            outs = {"out": _own(gd["out"]), "part": _own(gd["part"])}
            keep += [y, tabs, outs]
            f.y, f.ld_y, f.off_y = fptr(y), y.shape[1], int(gd.get("off_y", 0))
            f.scale, f.shift, f.mean, f.invstd = (fptr(tabs[k]) for k in ("scale", "shift", "mean", "invstd"))
            f.out, f.ld_out, f.off_out = fptr(outs["out"]), outs["out"].shape[1], int(gd.get("off_out", 0))
            f.part, f.part_rows = fptr(outs["part"]), outs["part"].shape[0]
            res["gates"].append(outs)
        a.raw_store, a.accum = (1 if raw_store else 0), (1 if accum else 0)
    names = C.create_string_buffer(16384)
    splits = (C.c_int * 2)()
    check(lib().p3d_debug_fused_conv(device, C.byref(a), names, len(names), splits))
    res.update(out=o, kernels=names.value.decode(), splits=(splits[0], splits[1]), gpart_rows=int(a.gpart_rows))
    return res


def fused_wgrad(problems, device=0):
    """Test hook: up to 6 filter gradients of fused-BatchNorm convs as ONE launch (p3d_debug_fused_wgrad).  Each problem is a dict:
    x [rows, ldx], offx, dy [rows, lddy], offdy, input_sizes, filter_sizes, strides, dw (what the gradient holds before; it is added
    to), dbias (or None), and optionally xt = 1 / 2 with xs1, xt1 (and x2 [rows, ldx2], offx2, xs2, xt2; the same array object as x
    shares its device buffer), dyt = 1 with dy2 [rows, lddy2], offdy2, dcoef [3, Cout].  Returns ([(dw, dbias or None), ...], kernel
    name, cuts, (slab stride, tile rows, tile columns))."""
    n = len(problems)
    cols = {k: [] for k in ("x", "dy", "x2", "xs1", "xt1", "xs2", "xt2", "dy2", "dcoef", "dw", "dbias")}
    ints = {k: [] for k in ("ldx", "offx", "lddy", "offdy", "xt", "ldx2", "offx2", "dyt", "lddy2", "offdy2")}
    xsh, wsh, st = [], [], []
    for pr in problems:
        fs = tuple(int(v) for v in pr["filter_sizes"])
        x, dy = _f32(pr["x"]), _f32(pr["dy"])
        x2 = x if pr.get("x2") is pr["x"] else (None if pr.get("x2") is None else _f32(pr["x2"]))
        dy2 = None if pr.get("dy2") is None else _f32(pr["dy2"])
        cols["x"].append(x); cols["dy"].append(dy); cols["x2"].append(x2); cols["dy2"].append(dy2)
        for k in ("xs1", "xt1", "xs2", "xt2", "dcoef"):
            cols[k].append(None if pr.get(k) is None else _f32(pr[k]))
        cols["dw"].append(_own(pr["dw"], fs))
        cols["dbias"].append(_own(pr.get("dbias")))
        ints["ldx"].append(x.shape[1]); ints["offx"].append(int(pr.get("offx", 0)))
        ints["lddy"].append(dy.shape[1]); ints["offdy"].append(int(pr.get("offdy", 0)))
        ints["xt"].append(int(pr.get("xt", 0))); ints["dyt"].append(int(pr.get("dyt", 0)))
        ints["ldx2"].append(0 if x2 is None else x2.shape[1]); ints["offx2"].append(int(pr.get("offx2", 0)))
        ints["lddy2"].append(0 if dy2 is None else dy2.shape[1]); ints["offdy2"].append(int(pr.get("offdy2", 0)))
        xsh += [int(v) for v in pr["input_sizes"]]
        wsh += list(fs)
        st += [int(v) for v in _strides3(pr["strides"])]
    fpp = type(fptr(cols["dw"][0]))
    arr = lambda k: (fpp * n)(*[fptr(v) for v in cols[k]])
    iv = lambda k: (C.c_int * n)(*ints[k])
    name = C.create_string_buffer(256)
    cuts, info = (C.c_int * n)(), (C.c_int * 3)()
    check(lib().p3d_debug_fused_wgrad(device, n, arr("x"), iv("ldx"), iv("offx"), (C.c_int64 * len(xsh))(*xsh), arr("dy"), iv("lddy"),
                                      iv("offdy"), (C.c_int64 * len(wsh))(*wsh), (C.c_int * len(st))(*st), iv("xt"), arr("x2"),
                                      iv("ldx2"), iv("offx2"), arr("xs1"), arr("xt1"), arr("xs2"), arr("xt2"), iv("dyt"), arr("dy2"),
                                      iv("lddy2"), iv("offdy2"), arr("dcoef"), arr("dw"), arr("dbias"), name, len(name), cuts, info))
    return list(zip(cols["dw"], cols["dbias"])), name.value.decode(), list(cuts), tuple(info)


def fused_reject(which, device=0):
    """Test hook (p3d_debug_fused_reject): (the launcher's hipError_t, whether the filter-gradient validator takes it) for malformed
    fused launch number `which`; hipErrorInvalidValue is 1."""
    err, ok = C.c_int(-1), C.c_int(-1)
    check(lib().p3d_debug_fused_reject(device, int(which), C.byref(err), C.byref(ok)))
    return err.value, bool(ok.value)


def perturb_selftest(mode="off", slow="producer", delay_us=200, with_wait=True, device=0):
    """Test hook (p3d_debug_perturb_selftest): a producer on one stream overwrites a buffer of 1.0 with 2.0, a consumer on another
    copies it out, with or without the wait between them, under P3DSession.perturb's `mode` ("slow": `slow` names whose stream is
    held back, "producer" | "consumer").  Returns the 4096 floats the consumer read."""
    out = np.empty(4096, np.float32)
    check(lib().p3d_debug_perturb_selftest(device, {"off": 0, "serial": 1, "slow": 2}[mode], {"producer": 0, "consumer": 1}[slow],
                                           int(delay_us), 1 if with_wait else 0, fptr(out)))
    return out


def max_pool3d_launch(x, ksize, strides, ld=(None, None), offset=(0, 0), pad=np.nan, prior=np.nan, device=0):
    """Test hook: tf.nn.max_pool3d SAME with x and y as channel slices (p3d_debug_max_pool3d); ld / offset = (of x, of y).
    Returns (y, what its buffer holds outside the slice)."""
    x = _f32(x)
    k, s = _strides3(ksize), _strides3(strides)
    C_ = x.shape[4]
    oshape = (x.shape[0],) + tuple(_same_out(x.shape[1 + i], s[i]) for i in range(3)) + (C_,)
    lx, ly = (C_ if v is None else int(v) for v in ld)
    xin = _embed(x.reshape(-1, C_), lx, offset[0], pad)
    rows = int(np.prod(oshape[:4]))
    y = _embed(np.broadcast_to(np.asarray(prior, np.float32), oshape).reshape(rows, C_), ly, offset[1], pad)
    check(lib().p3d_debug_max_pool3d(device, fptr(xin), lx, int(offset[0]), _shape5(x.shape), _i3(k), _i3(s), fptr(y), ly, int(offset[1])))
    return y[:, offset[1]:offset[1] + C_].reshape(oshape).copy(), _outside(y, C_, offset[1])


def max_pool3d_grad_launch(x, ksize, strides, grad, accumulate=False, ld=(None, None), offset=(0, 0), pad=np.nan, prior=np.nan, device=0):
    """Test hook: the gradient of max_pool3d_launch (p3d_debug_max_pool3d_grad); ld / offset = (of x and dx, of y and dy).  prior:
    what dx holds before; accumulate: the kernel adds to it.  Returns (dx, what its buffer holds outside the slice, kernel)."""
    x, g = _f32(x), _f32(grad)
    k, s = _strides3(ksize), _strides3(strides)
    C_ = x.shape[4]
    lx, ly = (C_ if v is None else int(v) for v in ld)
    rows = int(np.prod(x.shape[:4]))
    xin = _embed(x.reshape(rows, C_), lx, offset[0], pad)
    gin = _embed(g.reshape(-1, C_), ly, offset[1], pad)
    dx = _embed(np.broadcast_to(np.asarray(prior, np.float32), x.shape).reshape(rows, C_), lx, offset[0], pad)
    kernel = C.c_char_p()
    check(lib().p3d_debug_max_pool3d_grad(device, fptr(xin), lx, int(offset[0]), _shape5(x.shape), _i3(k), _i3(s), fptr(gin), ly,
                                          int(offset[1]), 1 if accumulate else 0, fptr(dx), C.byref(kernel)))
    return dx[:, offset[0]:offset[0] + C_].reshape(x.shape).copy(), _outside(dx, C_, offset[0]), kernel.value.decode()


def bias_add_grad_launch(dy, ld=None, offset=0, pad=np.nan, prior=0.0, device=0):
    """Test hook: BiasAddGrad on a channel slice of rows of `ld` floats, ADDED to `prior` (p3d_debug_bias_add_grad)."""
    g = _f32(dy)
    c = g.shape[-1]
    l = c if ld is None else int(ld)
    gin = _embed(g.reshape(-1, c), l, offset, pad)
    out = np.broadcast_to(np.asarray(prior, np.float32), (c,)).copy()
    check(lib().p3d_debug_bias_add_grad(device, fptr(gin), gin.shape[0], c, l, int(offset), fptr(out)))
    return out


def head(x, k, bias, dlogits, transpose=True, sigmoid=True, dk=None, dbias=None, fwd_path=0, filter_path=0, device=0):
    """Test hook: the network's output head (include/p3d_hip.h p3d_debug_head) on x [N, D, H, W, C]: transpose = the
    conv3d_transpose(x, 1, 3, 2) head, else the stride-1 conv3d(x, 1, 3, 1).  k: 27 * C floats ([3, 3, 3, 1, C] or
    [3, 3, 3, C, 1]); dlogits [N, D', H', W'].  dk, dbias: the gradients to add to (None: zeros).  fwd_path / filter_path:
    0 = the network's rule, else a forced kernel.  Returns (logits, pred, dx, dk [27, C], dbias (float32), (forward kernel,
    its blocks, filter-gradient kernel, its blocks))."""
    x = _f32(x)
    N, D, H, W, C_ = x.shape
    up = 2 if transpose else 1
    oshape = (N, up * D, up * H, up * W)
    logits, pred = np.empty(oshape, np.float32), np.empty(oshape, np.float32)
    dx = np.empty(x.shape, np.float32)
    dkk = np.zeros((27, C_), np.float32) if dk is None else _f32(np.asarray(dk).reshape(27, C_)).copy()
    db = np.zeros(1, np.float32) if dbias is None else _f32(np.asarray(dbias).reshape(1)).copy()
    info = (C.c_int * 4)()
    check(lib().p3d_debug_head(device, 1 if transpose else 0, N, D, H, W, C_, fptr(x), fptr(_f32(np.asarray(k).reshape(27, C_))),
                               fptr(_f32(np.asarray(bias).reshape(1))), 1 if sigmoid else 0, fptr(_f32(np.asarray(dlogits).reshape(oshape))),
                               int(fwd_path), int(filter_path), fptr(logits), fptr(pred), fptr(dx), fptr(dkk), fptr(db), info))
    return logits, pred, dx, dkk, db[0], tuple(info)


def smooth_l1(pred, target, through_sigmoid=True, offset=0, loss=0.0, device=0):
    """Test hook: the network's Smooth-L1 loss (p3d_debug_smooth_l1) on flat float32 pred / target placed `offset` elements
    into the device buffers.  Returns (loss + the sum, in double; dL/dlogits; (path taken: 1 float4 / 2 scalar, blocks))."""
    p, t = _f32(pred).ravel(), _f32(target).ravel()
    if p.size != t.size:
        raise ValueError("pred and target differ in size")
    dl = np.empty(p.size, np.float32)
    acc = C.c_double(float(loss))
    info = (C.c_int * 2)()
    check(lib().p3d_debug_smooth_l1(device, fptr(p), fptr(t), p.size, 1 if through_sigmoid else 0, int(offset), C.byref(acc),
                                    fptr(dl), info))
    return acc.value, dl, tuple(info)


def loss(kind, logits, pred, target, through_sigmoid=True, offset=0, loss=0.0, device=0):
    """Test hook: the network's selectable loss (p3d_debug_loss) of kind "smooth_l1" | "bce" | "l1" (or its P3D_LOSS_*
    number) on flat float32 logits / pred / target placed `offset` elements into the device buffers; pred is sigmoid(logits)
    when through_sigmoid, else the logits again.  Returns (loss + the sum, in double; dL/dlogits; (path taken: 1 float4 /
    2 scalar, blocks))."""
    k = LOSSES[kind] if isinstance(kind, str) else int(kind)
    z, p, t = _f32(logits).ravel(), _f32(pred).ravel(), _f32(target).ravel()
    if not (z.size == p.size == t.size):
        raise ValueError("logits, pred and target differ in size")
    dl = np.empty(p.size, np.float32)
    acc = C.c_double(float(loss))
    info = (C.c_int * 2)()
    check(lib().p3d_debug_loss(device, k, fptr(z), fptr(p), fptr(t), p.size, 1 if through_sigmoid else 0, int(offset),
                               C.byref(acc), fptr(dl), info))
    return acc.value, dl, tuple(info)


def map_loss(logits, pred, target, maps, map_elems, through_sigmoid=True, offset=0, kld_weight=1.0, cc_weight=1.0, loss=0.0,
             device=0):
    """Test hook: the per-map loss P3D_LOSS_KLD_CC as the network launches it (p3d_debug_map_loss) on `maps` maps of map_elems
    consecutive elements of flat float32 logits / pred / target, placed `offset` elements into the device buffers; s = pred
    when through_sigmoid, else sigmoid(logits).  Returns (loss + the weighted sum, in double; dL/dlogits; per_map [maps, 2] =
    KL_m, CC_m (NaN where CC is undefined); (launches, blocks per map, path taken: 1 float4 / 2 scalar))."""
    z, t = _f32(logits).ravel(), _f32(target).ravel()
    p = _f32(pred).ravel() if pred is not None else z
    n = int(maps) * int(map_elems)
    if not (z.size == p.size == t.size == n):
        raise ValueError("logits, pred and target must hold maps * map_elems elements")
    dl = np.empty(n, np.float32)
    per_map = np.empty((int(maps), 2), np.float64)
    acc = C.c_double(float(loss))
    info = (C.c_int * 3)()
    check(lib().p3d_debug_map_loss(device, fptr(z), fptr(p), fptr(t), int(maps), int(map_elems), 1 if through_sigmoid else 0,
                                   int(offset), float(kld_weight), float(cc_weight), C.byref(acc), fptr(dl),
                                   per_map.ctypes.data_as(C.POINTER(C.c_double)), info))
    return acc.value, dl, per_map, tuple(info)


def saliency_loss(logits, pred, target, fixations, maps, map_elems, through_sigmoid=True, offset=0, kld_weight=1.0, cc_weight=1.0,
                  nss_weight=1.0, sim_weight=0.0, loss=0.0, device=0):
    """Test hook: the per-map loss P3D_LOSS_SALIENCY as the network launches it (p3d_debug_saliency_loss): map_loss with the
    uint8 fixation bytes `fixations` (fixated where >= 128; None only with nss_weight 0, when they are not read), placed `offset`
    bytes into their device buffer, and the four weights.  Returns (loss + the weighted sum, in double; dL/dlogits; per_map
    [maps, 4] = KL_m, CC_m, NSS_m, SIM_m (NaN where undefined); (launches, blocks per map, path taken: 1 float4 / 2 scalar))."""
    z, t = _f32(logits).ravel(), _f32(target).ravel()
    p = _f32(pred).ravel() if pred is not None else z
    n = int(maps) * int(map_elems)
    if not (z.size == p.size == t.size == n):
        raise ValueError("logits, pred and target must hold maps * map_elems elements")
    f = None
    if fixations is not None:
        f = np.ascontiguousarray(fixations).ravel()
        if f.dtype != np.uint8 or f.size != n:
            raise ValueError("fixations must be maps * map_elems uint8 bytes")
    dl = np.empty(n, np.float32)
    per_map = np.empty((int(maps), 4), np.float64)
    acc = C.c_double(float(loss))
    info = (C.c_int * 3)()
    check(lib().p3d_debug_saliency_loss(device, fptr(z), fptr(p), fptr(t), f.ctypes.data_as(C.POINTER(C.c_ubyte)) if f is not None else None,
                                        int(maps), int(map_elems), 1 if through_sigmoid else 0, int(offset), float(kld_weight),
                                        float(cc_weight), float(nss_weight), float(sim_weight), C.byref(acc), fptr(dl),
                                        per_map.ctypes.data_as(C.POINTER(C.c_double)), info))
    return acc.value, dl, per_map, tuple(info)


def _opt_scaled(kind, p, g, m, v, tiles, t, lr, b1, b2, eps, momentum, use_nesterov, lr_on_device, gscale, offset, device):
    """p3d_debug_opt_scaled on copies already made: any optimiser launch with clipping's scale.  Returns (term, step size)."""
    i64 = C.POINTER(C.c_int64)
    offs = lens = cs = None
    if tiles is not None:
        lens = np.array([int(n) for n, _ in tiles], np.int64)
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        cs = np.array([c for _, c in tiles], np.float32)
    term, lr_t = C.c_double(), C.c_float()
    check(lib().p3d_debug_opt_scaled(device, int(kind), fptr(p), fptr(g), fptr(m), fptr(v), p.size, int(offset),
                                     offs.ctypes.data_as(i64) if tiles is not None else None,
                                     lens.ctypes.data_as(i64) if tiles is not None else None, fptr(cs),
                                     len(tiles) if tiles is not None else 0, float(lr), int(t), float(b1), float(b2), float(eps),
                                     float(momentum), 1 if use_nesterov else 0, 1 if lr_on_device else 0,
                                     float(np.float32(gscale)), C.byref(term), C.byref(lr_t)))
    return term.value, lr_t.value


def adam(p, g, m, v, t, lr=1e-4, b1=0.9, b2=0.999, eps=1e-8, lr_on_device=False, offset=0, device=0, gscale=None):
    """Test hook: one launch of the network's Adam kernel (p3d_debug_adam) on flat float32 arrays, step t (1-based).  Returns
    (p, m, v after the step, the float32 step size lr * sqrt(1 - b2^t) / (1 - b1^t) it used).  gscale: clipping's float32
    scale, read from device memory; the step runs on float32(g * gscale) (adam_scaled_kernel)."""
    p, m, v = (_f32(a).ravel().copy() for a in (p, m, v))
    g = _f32(g).ravel()
    if not (p.size == g.size == m.size == v.size):
        raise ValueError("p, g, m, v differ in size")
    if gscale is not None:
        _, step = _opt_scaled(OPTIMIZERS["adam"], p, g.copy(), m, v, None, t, lr, b1, b2, eps, 0.0, False, lr_on_device, gscale, offset,
                              device)
        return p, m, v, step
    lr_t = C.c_float()
    check(lib().p3d_debug_adam(device, fptr(p), fptr(g), fptr(m), fptr(v), p.size, int(offset), float(lr), int(t), float(b1),
                               float(b2), float(eps), 1 if lr_on_device else 0, C.byref(lr_t)))
    return p, m, v, lr_t.value


def adam_decay(p, g, m, v, tiles, t, lr=1e-4, b1=0.9, b2=0.999, eps=1e-8, lr_on_device=False, update=True, offset=0, device=0,
               gscale=None):
    """Test hook: one launch of the regularised optimiser step (p3d_debug_adam_decay) on flat float32 arrays.  tiles = [(length,
    coefficient), ...] cut [0, n) in order; each gets one float32 coefficient c, and g' = g + c p.  With update, p, m, v take
    Adam's step t on g'; without, only g changes.  Returns (g', p, m, v, the term sum 0.5 c sum(p^2) in double, the float32
    step size).  gscale: clipping's scale; the step runs on float32(g' * gscale), g' comes back unscaled."""
    p, g, m, v = (_f32(a).ravel().copy() for a in (p, g, m, v))
    if not (p.size == g.size == m.size == v.size):
        raise ValueError("p, g, m, v differ in size")
    if gscale is not None:
        if not update:
            raise ValueError("gscale: the gradient-only launch scales nothing")
        term, step = _opt_scaled(OPTIMIZERS["adam"], p, g, m, v, tiles, t, lr, b1, b2, eps, 0.0, False, lr_on_device, gscale, offset,
                                 device)
        return g, p, m, v, term, step
    lens = np.array([int(n) for n, _ in tiles], np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    cs = np.array([c for _, c in tiles], np.float32)
    i64 = C.POINTER(C.c_int64)
    term, lr_t = C.c_double(), C.c_float()
    check(lib().p3d_debug_adam_decay(device, fptr(p), fptr(g), fptr(m), fptr(v), p.size, int(offset), offs.ctypes.data_as(i64),
                                     lens.ctypes.data_as(i64), fptr(cs), len(tiles), float(lr), int(t), float(b1), float(b2),
                                     float(eps), 1 if lr_on_device else 0, 1 if update else 0, C.byref(term), C.byref(lr_t)))
    return g, p, m, v, term.value, lr_t.value


def _opt_kind(kind):
    k = OPTIMIZERS[kind] if isinstance(kind, str) else int(kind)
    if k not in (OPTIMIZERS["momentum"], OPTIMIZERS["sgd"]):
        raise ValueError("optimizer %r: the hooks take momentum or sgd (Adam has adam / adam_decay)" % (kind,))
    return k


def optimizer(kind, p, g, m, lr=1e-4, momentum=0.9, use_nesterov=False, lr_on_device=False, offset=0, device=0, gscale=None):
    """Test hook: one launch of the Momentum or SGD step (p3d_debug_optimizer, kind "momentum" | "sgd") on flat float32 arrays
    placed `offset` elements into the device buffers; m is Momentum's accumulator.  Returns (p, m) after the step.  gscale:
    clipping's scale; the step runs on float32(g * gscale)."""
    k = _opt_kind(kind)
    p, g, m = (_f32(a).ravel().copy() for a in (p, g, m))
    if not (p.size == g.size == m.size):
        raise ValueError("p, g, m differ in size")
    if gscale is not None:
        _opt_scaled(k, p, g, m, np.zeros_like(p), None, 1, lr, 0.0, 0.0, 0.0, momentum, use_nesterov, lr_on_device, gscale, offset, device)
        return p, m
    check(lib().p3d_debug_optimizer(device, k, fptr(p), fptr(g), fptr(m), p.size, int(offset), float(lr), float(momentum),
                                    1 if use_nesterov else 0, 1 if lr_on_device else 0))
    return p, m


def ema(s, p, om, om_on_device=False, offset=0, device=0):
    """Test hook: one launch of the moving-average kernel of P3DSession.set_ema (ema_kernel, p3d_debug_ema) on flat float32
    shadows s and parameters p placed `offset` (0..3) elements past a 16-byte boundary; om is float32(1 - decay), passed as an
    argument or through device memory.  Returns s - (s - p) * om.  The hook itself guards both sides of the range."""
    s = _f32(s).ravel().copy()
    p = _f32(p).ravel()
    if s.size != p.size:
        raise ValueError("s and p differ in size")
    check(lib().p3d_debug_ema(device, fptr(s), fptr(p), s.size, int(offset), float(np.float32(om)), 1 if om_on_device else 0))
    return s


GRAD_ACCUM_MODES = {"store": 0, "add": 1, "finish": 2}


def grad_accum(acc, g, mode, offset=0, device=0):
    """Test hook: one launch of the accumulation kernel of P3DSession.set_grad_accum (grad_accum_kernel, p3d_debug_grad_accum)
    on a flat float32 accumulator acc and gradient g placed `offset` (0..3) elements past a 16-byte boundary.  mode "store":
    acc = g; "add": acc = acc + g; "finish": g = acc + g.  Returns the operand the mode writes; the inputs are not modified.
    The hook itself guards both sides of the range and checks that the other operand kept its bits."""
    acc = _f32(acc).ravel().copy()
    g = _f32(g).ravel().copy()
    if acc.size != g.size:
        raise ValueError("acc and g differ in size")
    m = GRAD_ACCUM_MODES[mode] if isinstance(mode, str) else int(mode)
    check(lib().p3d_debug_grad_accum(device, m, fptr(acc), fptr(g), acc.size, int(offset)))
    return g if m == 2 else acc


def augment(x, y, fix, decisions, offset=0, device=0):
    """Test hook: the augmentation launches of P3DSession.set_augment (p3d_debug_augment) with explicit per-clip decisions
    [(flip, reverse, y0, x0, ch, cw, a, b), ...] on x [B,T,H,W,3], y [B,T,H,W] float32 and fix [B,T,H,W] uint8 (or None), every
    device buffer `offset` (0..3) elements past a 16-byte boundary.  Returns (x', y', fix' or None); the inputs are not modified.
    The hook itself guards both sides of every output and checks that the inputs kept their bits."""
    x, y = _f32(x), _f32(y)
    if x.ndim != 5 or x.shape[4] != 3 or y.shape != x.shape[:4]:
        raise ValueError("x is [B,T,H,W,3] and y [B,T,H,W]")
    B, T, H, W = y.shape
    u8 = C.POINTER(C.c_ubyte)
    f = fo = None
    if fix is not None:
        f = np.ascontiguousarray(fix)
        if f.dtype != np.uint8 or f.shape != y.shape:
            raise ValueError("fix is uint8 [B,T,H,W]")
        fo = np.empty_like(f)
    d = list(decisions)
    if len(d) != B:
        raise ValueError("one row of decisions per clip")
    geom = np.ascontiguousarray([[int(v) for v in r[:6]] for r in d], dtype=np.int32)
    photo = np.ascontiguousarray([[r[6], r[7]] for r in d], dtype=np.float32)
    xo, yo = np.empty_like(x), np.empty_like(y)
    check(lib().p3d_debug_augment(device, fptr(x), fptr(y), f.ctypes.data_as(u8) if f is not None else None, B, T, H, W,
                                  geom.ctypes.data_as(C.POINTER(C.c_int32)), fptr(photo), int(offset), fptr(xo), fptr(yo),
                                  fo.ctypes.data_as(u8) if fo is not None else None))
    return xo, yo, fo


def augment_draw(seed, g, H, W, flip=0., reverse=0., min_scale=1., contrast=0., brightness=0.):
    """Host only: the decisions (flip, reverse, y0, x0, ch, cw, a, b) P3DSession.set_augment's settings give clip g (global index)
    under `seed` on an H x W grid (p3d_debug_augment_draw); a and b are numpy float32."""
    from ._lib import P3dAugment
    cfg = P3dAugment(float(flip), float(reverse), float(min_scale), float(contrast), float(brightness))
    geom, photo = (C.c_int32 * 6)(), (C.c_float * 2)()
    check(lib().p3d_debug_augment_draw(int(seed), int(g), int(H), int(W), C.byref(cfg), geom, photo))
    return (bool(geom[0]), bool(geom[1]), geom[2], geom[3], geom[4], geom[5], np.float32(photo[0]), np.float32(photo[1]))


def optimizer_decay(kind, p, g, m, tiles, lr=1e-4, momentum=0.9, use_nesterov=False, lr_on_device=False, update=True, offset=0,
                    device=0, gscale=None):
    """Test hook: adam_decay's launch with Momentum or SGD as the update (p3d_debug_optimizer_decay).  tiles = [(length,
    coefficient), ...] cut [0, n) in order, g' = g + c p.  Returns (g', p, m, the term sum 0.5 c sum(p^2) in double).  gscale:
    clipping's scale; the step runs on float32(g' * gscale), g' comes back unscaled."""
    k = _opt_kind(kind)
    p, g, m = (_f32(a).ravel().copy() for a in (p, g, m))
    if not (p.size == g.size == m.size):
        raise ValueError("p, g, m differ in size")
    if gscale is not None:
        if not update:
            raise ValueError("gscale: the gradient-only launch scales nothing")
        term, _ = _opt_scaled(k, p, g, m, np.zeros_like(p), tiles, 1, lr, 0.0, 0.0, 0.0, momentum, use_nesterov, lr_on_device, gscale,
                              offset, device)
        return g, p, m, term
    lens = np.array([int(n) for n, _ in tiles], np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    cs = np.array([c for _, c in tiles], np.float32)
    i64 = C.POINTER(C.c_int64)
    term = C.c_double()
    check(lib().p3d_debug_optimizer_decay(device, k, fptr(p), fptr(g), fptr(m), p.size, int(offset), offs.ctypes.data_as(i64),
                                          lens.ctypes.data_as(i64), fptr(cs), len(tiles), float(lr), float(momentum),
                                          1 if use_nesterov else 0, 1 if lr_on_device else 0, 1 if update else 0, C.byref(term)))
    return g, p, m, term.value


GRAD_NORM_CHUNK = 8192      # the cut of the flat gradient range (REG_TILE of the network)


def grad_norm(g, clip_norm, p=None, tiles=None, ranges=None, offset=0, blocks=0, device=0):
    """Test hook: the global-norm reduction of P3DSession.set_grad_clip (grad_sumsq_kernel, p3d_debug_grad_norm) on a flat
    float32 gradient placed `offset` (0..3) elements into the device buffer.  tiles = [(length, coefficient), ...] cut [0, n) in
    order: a tile with a float coefficient c is one chunk on which g' = float32(g + float32(c p)) (p is needed when any c != 0);
    a tile whose coefficient is None is slot padding, which belongs to no chunk and is never read.  Without tiles, [0, n) is cut
    every GRAD_NORM_CHUNK elements with c = 0.  ranges = [(lo, hi), ...] are launched in that order, the last one folding
    (default: one launch over everything); each must start and end between chunks.  blocks caps the grid (0: the step's cap).
    Returns (sumsq, norm) in float64 and the float32 scale = clip_norm / max(norm, clip_norm) (1 under inf, NaN when the norm is
    not finite)."""
    g = _f32(g).ravel()
    n = g.size
    if p is not None:
        p = _f32(p).ravel()
        if p.size != n:
            raise ValueError("g and p differ in size")
    if tiles is None:
        tiles = [(min(GRAD_NORM_CHUNK, n - a), 0.0) for a in range(0, n, GRAD_NORM_CHUNK)]
    offs, lens, cs, at = [], [], [], 0
    for length, c in tiles:
        if c is not None:
            offs.append(at); lens.append(int(length)); cs.append(c)
        at += int(length)
    if at != n:
        raise ValueError("tiles must cover [0, n)")
    offs, lens, cs = np.array(offs, np.int64), np.array(lens, np.int64), np.array(cs, np.float32)
    ranges = [(0, n)] if ranges is None else list(ranges)
    lo = np.array([int(a) for a, _ in ranges], np.int64)
    hi = np.array([int(b) for _, b in ranges], np.int64)
    i64 = C.POINTER(C.c_int64)
    ss, nm, sc = C.c_double(), C.c_double(), C.c_float()
    check(lib().p3d_debug_grad_norm(device, fptr(g), fptr(p), n, int(offset), offs.ctypes.data_as(i64), lens.ctypes.data_as(i64),
                                    fptr(cs), len(offs), lo.ctypes.data_as(i64), hi.ctypes.data_as(i64), len(ranges),
                                    float(np.float32(clip_norm)), int(blocks), C.byref(ss), C.byref(nm), C.byref(sc)))
    return ss.value, nm.value, np.float32(sc.value)


def stat_parts(xshape, fshape, strides, transpose=False):
    """Host-only test hook: (partials the conv's statistics epilogue writes, room the network reserves for them)."""
    w, c = C.c_int(), C.c_int()
    check(lib().p3d_debug_stat_parts(_shape5(xshape), _shape5(fshape), _i3(_strides3(strides)), 1 if transpose else 0,
                                     C.byref(w), C.byref(c)))
    return w.value, c.value


def igemm_groupable(xshape, fshape, strides):
    """Host-only test hook: would two sibling convs of this shape on one input go out as one grouped launch?"""
    r = lib().p3d_debug_igemm_groupable(_shape5(xshape), _shape5(fshape), _i3(_strides3(strides)))
    check(-1 if r < 0 else 0)
    return bool(r)


def bias_add_grad(dy, device=0):
    """BiasAddGrad (gradient of the bias of tf.layers.conv3d / conv3d_transpose): sum of dy over every axis but the last."""
    g = _f32(dy)
    c = g.shape[-1]
    out = np.empty((c,), np.float32)
    check(lib().p3d_op_bias_add_grad(device, fptr(g), g.size // c if c else 0, c, fptr(out)))
    return out


def attention_core(g, f, h, d_o=None, device=0):
    """utils/network.py:183-185 on flattened operands: o = softmax(g f^T) h for g [B, Ng, ch/8], f [B, Nf, ch/8], h [B, Nf, ch]
    (ch in 32, 64, 128, 256), the score matrix never stored.  With d_o (gradient of o): returns (o, dg, df, dh)."""
    g, f, h = _f32(g), _f32(f), _f32(h)
    B, ng, ci = g.shape
    nf, ch = h.shape[1], h.shape[2]
    if f.shape != (B, nf, ci) or h.shape[0] != B or ci * 8 != ch:
        raise ValueError("attention_core: g [B,Ng,ch/8], f [B,Nf,ch/8], h [B,Nf,ch]")
    o = np.empty((B, ng, ch), np.float32)
    if d_o is None:
        check(lib().p3d_op_attention_core(device, B, ng, nf, ch, fptr(g), fptr(f), fptr(h), fptr(o), None, None, None, None))
        return o
    d = _f32(d_o)
    if d.shape != o.shape:
        raise ValueError("attention_core: d_o has the shape of o")
    dg, df, dh = np.empty_like(g), np.empty_like(f), np.empty_like(h)
    check(lib().p3d_op_attention_core(device, B, ng, nf, ch, fptr(g), fptr(f), fptr(h), fptr(o), fptr(d), fptr(dg), fptr(df), fptr(dh)))
    return o, dg, df, dh


ATTENTION_MODES = {"stored": 1, "flash": 2}


def attention_core_launch(mode, g, f, h, d_o=None, device=0):
    """Test hook (p3d_debug_attention_core): attention_core in the execution `mode` -- "stored": the graph op's launch sequence
    around a stored score matrix (any ch that is a multiple of 32), "flash": the kernels of attention_core.  Outputs and scratch
    hold NaNs before the launches."""
    g, f, h = _f32(g), _f32(f), _f32(h)
    B, ng, ci = g.shape
    nf, ch = h.shape[1], h.shape[2]
    if f.shape != (B, nf, ci) or h.shape[0] != B or ci * 8 != ch:
        raise ValueError("attention_core_launch: g [B,Ng,ch/8], f [B,Nf,ch/8], h [B,Nf,ch]")
    m = ATTENTION_MODES[mode]
    o = np.empty((B, ng, ch), np.float32)
    if d_o is None:
        check(lib().p3d_debug_attention_core(device, m, B, ng, nf, ch, fptr(g), fptr(f), fptr(h), fptr(o), None, None, None, None))
        return o
    d = _f32(d_o)
    if d.shape != o.shape:
        raise ValueError("attention_core_launch: d_o has the shape of o")
    dg, df, dh = np.empty_like(g), np.empty_like(f), np.empty_like(h)
    check(lib().p3d_debug_attention_core(device, m, B, ng, nf, ch, fptr(g), fptr(f), fptr(h), fptr(o), fptr(d), fptr(dg), fptr(df),
                                         fptr(dh)))
    return o, dg, df, dh


def attention_splits(B, ng, nf, ch):
    """Host-only test hook: K-slices of the four row-major products of the stored-score execution (g f^T, beta h, d_o h^T, ds f)."""
    sp = (C.c_int * 4)()
    check(lib().p3d_debug_attention_splits(B, ng, nf, ch, sp))
    return tuple(sp)


def softmax_rows_launch(s, cols, d=None, guard_rows=0, device=0):
    """Test hook (p3d_debug_softmax_rows) on whole buffers [rows + guard_rows, ld]: the softmax over the first `cols` columns of the
    first `rows` rows of `s` (d = None; returns the buffer after the launch), or its gradient from the attention map `s` and the
    map's gradient `d` (returns d's buffer after the launch)."""
    s = _f32(s).copy()
    rows, ld = s.shape[0] - guard_rows, s.shape[1]
    if d is None:
        check(lib().p3d_debug_softmax_rows(device, 0, rows, cols, ld, fptr(s), None, guard_rows))
        return s
    d = _f32(d).copy()
    if d.shape != s.shape:
        raise ValueError("softmax_rows_launch: d has the shape of s")
    check(lib().p3d_debug_softmax_rows(device, 1, rows, cols, ld, fptr(s), fptr(d), guard_rows))
    return d


def attn_mix(r, x, gamma, C_, offset=(0, 0, 0), drop_rate=0.0, seed=0, seed_dev=False, z=None, dz=None, accx=False, dr=None, dx=None,
             dgamma=0.0, device=0):
    """Test hook (p3d_debug_attn_mix): z = r * gamma + x on `C_` channels at the column offsets (of r, of x, of z) of the wide
    buffers r [M, ldr], x [M, ldx], z [M, ldz] (what z holds before the launch; default: dense, NaN), the block's dropout, and with dz
    [M, ldz] the backward pass into dr [M, ldr] and dx [M, ldx] (what they hold before; accx: dx is added to) and dgamma (added
    to).  Returns the z buffer, or (z, dr, dx, dgamma) buffers."""
    r, x = _f32(r), _f32(x)
    M = r.shape[0]
    z = np.full((M, int(C_)), np.nan, np.float32) if z is None else _f32(z).copy()
    args = (device, M, int(C_), fptr(r), r.shape[1], int(offset[0]), fptr(x), x.shape[1], int(offset[1]), float(gamma), float(drop_rate),
            int(seed), 1 if seed_dev else 0, fptr(z), z.shape[1], int(offset[2]))
    if dz is None:
        check(lib().p3d_debug_attn_mix(*args, None, 0, None, None, None))
        return z
    dz = _f32(dz)
    dr = np.full(r.shape, np.nan, np.float32) if dr is None else _f32(dr).copy()
    dx = np.full(x.shape, np.nan, np.float32) if dx is None else _f32(dx).copy()
    dgm = np.array([dgamma], np.float32)
    if dz.shape != z.shape or dr.shape != r.shape or dx.shape != x.shape:
        raise ValueError("attn_mix: dz, dr, dx have the shapes of z, r, x")
    check(lib().p3d_debug_attn_mix(*args, fptr(dz), 1 if accx else 0, fptr(dr), fptr(dx), fptr(dgm)))
    return z, dr, dx, dgm[0]


def max_pool3d(x, ksize, strides, padding="SAME", device=0):
    """tf.nn.max_pool3d(x, [1,kd,kh,kw,1], [1,sd,sh,sw,1], 'SAME')."""
    x = _f32(x)
    k, s = _strides3(ksize), _strides3(strides)
    y = np.empty((x.shape[0],) + tuple(_same_out(x.shape[1 + i], s[i]) for i in range(3)) + (x.shape[4],), np.float32)
    check(lib().p3d_op_max_pool3d(device, fptr(x), _shape5(x.shape), _i3(k), _i3(s), fptr(y)))
    return y


def max_pool3d_grad(x, ksize, strides, grad, device=0):
    x, g = _f32(x), _f32(grad)
    k, s = _strides3(ksize), _strides3(strides)
    dx = np.empty(x.shape, np.float32)
    check(lib().p3d_op_max_pool3d_grad(device, fptr(x), _shape5(x.shape), _i3(k), _i3(s), fptr(g), fptr(dx)))
    return dx
