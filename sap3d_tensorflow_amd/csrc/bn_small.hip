// BatchNorm for SMALL tensors (M = B*D*H*W <= 1024 rows: every layer of stage 3 at batch 8) on
// gfx950: statistics + normalise + ReLU + residual in ONE launch, and the whole backward in ONE
// launch.  tf.layers.batch_normalization on rank-5 input is per-channel, so a block that owns 4
// channels needs no other block: it keeps its [M x 4] slab in REGISTERS (4 float4 per thread per
// tensor), reduces with wave shuffles + a 4-entry LDS exchange, and writes the result.  No atomics,
// no statistics arena, no finalize launch; variance is the two-pass form TF's tf.nn.moments uses.
// Modes are those of bn_apply_kernel (p3d_kernels.h); reference p3d.py:56-81,88,114,127,133-134.
// A channel's summation order is that of the 8- / 16-channel slabs these kernels began with (dispatch, chain_sum2).
// Which slab a block owns goes through xcd_slab(): the blocks of one XCD own a contiguous run of slabs, so the 8 slabs
// that share a 128-byte line of a row are read and written through ONE L2 (speed only, see there).
#include "p3d_kernels.h"
#include <cstdlib>

namespace {

constexpr int CB = 8;          // smallest channel slab whose summation order dispatch uses (8 or 16), and the granule the path takes

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float4 f4(float a) { return make_float4(a, a, a, a); }
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 sub4(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
__device__ __forceinline__ float4 mul4(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float4 fma4(float4 a, float4 b, float4 c) {
    return make_float4(fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y), fmaf(a.z, b.z, c.z), fmaf(a.w, b.w, c.w));
}
// relu(NaN) is NaN (fmaxf would return the 0); finite values and -0.f give the bits fmaxf gave
__device__ __forceinline__ float relu1(float v) { return v > 0.f ? v : (v != v ? v : 0.f); }
__device__ __forceinline__ float4 relu4(float4 a) { return make_float4(relu1(a.x), relu1(a.y), relu1(a.z), relu1(a.w)); }
__device__ __forceinline__ float4 gate4(float4 g, float4 pre) {
    return make_float4(pre.x > 0.f ? g.x : 0.f, pre.y > 0.f ? g.y : 0.f, pre.z > 0.f ? g.z : 0.f, pre.w > 0.f ? g.w : 0.f);
}
__device__ __forceinline__ float4 shfl4(float4 v, int o) {
    return make_float4(__shfl_xor(v.x, o), __shfl_xor(v.y, o), __shfl_xor(v.z, o), __shfl_xor(v.w, o));
}

#if defined(P3D_TUNING)
__device__ int g_bn_slab_identity;      // P3D_BN_XCD=0 (tuning build): slab = block index, for the A/B of xcd_slab() on the same kernels
#endif

// Block -> channel slab, a bijection on [0, nb).  Blocks are dealt round-robin over the 8 XCDs, each with its own L2, so
// with slab = block index the 2 / 4 / 8 slabs (64 / 32 / 16 bytes of a row) that share one 128-byte line sit on as many
// XCDs: each fetches the line from beyond its L2 and writes it back in parts.  Here the blocks with equal b % 8 own a
// contiguous run of nb/8 (+1 for the first nb%8 of them) slabs -- C = 256 in 8-channel slabs: one whole line per row and
// XCD.  Grids below 8 blocks keep the identity.  Nothing but speed depends on where the hardware puts a block, and a
// channel's sum tree does not depend on which block owns it, so the results are those of the identity order bit for bit.
// Measured with tools/micro/bn_chain (P3D_BN_XCD=0/1 per P3D_BN_CB, profiles/r16_bn_chain.log; EXPERIMENTS.md).
__device__ __forceinline__ int xcd_slab(int b, int nb) {
#if defined(P3D_TUNING)
    if (g_bn_slab_identity) return b;
#endif
    if (nb < 8) return b;
    const int x = b & 7, q = nb >> 3, r = nb & 7;
    return x * q + min(x, r) + (b >> 3);
}

__device__ __forceinline__ float4 shfl_up4(float4 v) {
    return make_float4(__shfl_up(v.x, 1), __shfl_up(v.y, 1), __shfl_up(v.z, 1), __shfl_up(v.w, 1));
}

// A thread's share of a channel's sum.  A CHAIN is the sequential sum over the rows  rowslot + RS * j, j = 0, 1, ...  of one row
// slot; which rows form a chain and how the chains are added (block_sum2) IS the channel's summation order.  With P > 1 a chain is
// walked by P neighbouring lanes, MJ rows each: lane h takes over the running sums of lane h - 1 and goes on with them, so the
// additions are those of one thread walking the chain, in the same order, bit for bit.  add(j, s, q) folds local row j into (s, q).
template <int P, int MJ, class F>
__device__ __forceinline__ void chain_sum2(float4& s, float4& q, int h, F add) {
#pragma unroll
    for (int p = 0; p < P; ++p) {
        if (h == p) {
#pragma unroll
            for (int j = 0; j < MJ; ++j) add(j, s, q);
        }
        if (p + 1 < P) {
            const float4 ts = shfl_up4(s), tq = shfl_up4(q);
            if (h == p + 1) { s = ts; q = tq; }
        }
    }
}

// Sums of `v` and `w` over the chains of the block, per channel quad; both broadcast back to every thread.  A row slot is G * P
// neighbouring lanes (G channel quads, or the P lanes of one split chain, whose last lane holds the chain's sums).
template <int G, int P>
__device__ __forceinline__ void block_sum2(float4& v, float4& w, float4* xch /*[2][4][G][2]*/, int phase) {
#pragma unroll
    for (int o = G * P; o < 64; o <<= 1) { v = add4(v, shfl4(v, o)); w = add4(w, shfl4(w, o)); }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = (threadIdx.x / P) % G;
    float4* slot = xch + (phase & 1) * 8 * G;
    if (lane < G * P && lane % P == P - 1) { slot[(wave * G + g) * 2] = v; slot[(wave * G + g) * 2 + 1] = w; }
    __syncthreads();
    v = add4(add4(slot[g * 2], slot[(G + g) * 2]), add4(slot[(2 * G + g) * 2], slot[(3 * G + g) * 2]));
    w = add4(add4(slot[g * 2 + 1], slot[(G + g) * 2 + 1]), add4(slot[(2 * G + g) * 2 + 1], slot[(3 * G + g) * 2 + 1]));
}

// One-pass mean / biased variance of the slab held in registers, shifted by the channel's first row so that
// E[d^2] - E[d]^2 does not cancel (d = x - x[0]).
template <int G, int P, int MJ>
__device__ __forceinline__ void bn_moments(const float4 (&v)[MJ], float4 shift, int nj, int M, int rowslot, int h, float4* xch,
                                           int& phase, float4& mean, float4& var) {
    constexpr int RS = 256 / (G * P);
    // a first row that is inf or NaN is no shift: x - inf would turn a mean of +inf (what the unshifted sums of the other paths and
    // the reference give) into NaN
    shift = make_float4(shift.x - shift.x == 0.f ? shift.x : 0.f, shift.y - shift.y == 0.f ? shift.y : 0.f,
                        shift.z - shift.z == 0.f ? shift.z : 0.f, shift.w - shift.w == 0.f ? shift.w : 0.f);
    float4 s = f4(0.f), q = f4(0.f);
    chain_sum2<P, MJ>(s, q, h, [&](int j, float4& s_, float4& q_) {
        if (h * MJ + j < nj && rowslot + RS * (h * MJ + j) < M) { const float4 d = sub4(v[j], shift); s_ = add4(s_, d); q_ = fma4(d, d, q_); }
    });
    block_sum2<G, P>(s, q, xch, phase++);
    const float invM = 1.f / (float)M;
    const float4 md = mul4(s, f4(invM));
    mean = add4(shift, md);
    var = sub4(mul4(q, f4(invM)), mul4(md, md));
    var = make_float4(fmaxf(var.x, 0.f), fmaxf(var.y, 0.f), fmaxf(var.z, 0.f), fmaxf(var.w, 0.f));
    // a sum of squares that is inf or NaN has no variance (inf - inf), and fmaxf would turn that NaN into 0: it stays NaN, as in
    // bn_finalize_kernel.  (Asked of q, not of var: a second use of the difference changes how the compiler contracts it, and
    // with it the bits of every finite variance.)
    var = make_float4(q.x - q.x == 0.f ? var.x : NAN, q.y - q.y == 0.f ? var.y : NAN, q.z - q.z == 0.f ? var.z : NAN,
                      q.w - q.w == 0.f ? var.w : NAN);
}

// The per-channel parameters a block needs, loaded TOGETHER WITH its data: read where they are used, behind the block-wide
// reduction, each of them is one more dependent trip to memory (~1.5 us of a 6-9 us launch).
struct BnChan { float4 gamma, beta, mm, mv; };
__device__ __forceinline__ BnChan bn_chan_load(const BnParams& bn, int c, bool need_moving) {
    BnChan p;
    p.gamma = ld4(bn.gamma + c); p.beta = ld4(bn.beta + c);
    p.mm = f4(0.f); p.mv = f4(1.f);
    if (need_moving) { p.mm = ld4(bn.moving_mean + c); p.mv = ld4(bn.moving_var + c); }
    return p;
}
__device__ __forceinline__ void bn_coeffs(const BnParams& bn, const BnChan& ch, int c, bool use_batch, bool update_moving, float eps, bool writer,
                                          float4& mean, float4& var, float4& scale, float4& shift) {
    if (!use_batch) { mean = ch.mm; var = ch.mv; }
    const float4 inv = make_float4(1.f / sqrtf(var.x + eps), 1.f / sqrtf(var.y + eps), 1.f / sqrtf(var.z + eps), 1.f / sqrtf(var.w + eps));
    scale = mul4(ch.gamma, inv);
    shift = sub4(ch.beta, mul4(mean, scale));
    if (writer) {
        st4(bn.scale + c, scale); st4(bn.shift + c, shift); st4(bn.mean + c, mean); st4(bn.invstd + c, inv);
        if (use_batch && update_moving) {     // moving -= (moving - batch) * (1 - 0.99), biased variance (Appendix A.4)
            st4(bn.moving_mean + c, sub4(ch.mm, mul4(sub4(ch.mm, mean), f4(1.0f - 0.99f))));
            st4(bn.moving_var + c, sub4(ch.mv, mul4(sub4(ch.mv, var), f4(1.0f - 0.99f))));
        }
    }
}

template <int MODE, int CBW, bool SPLIT>
__global__ __launch_bounds__(256) void bn_small_fwd_kernel(BnSmallArgs a) {
    P3D_CHAIN_PRIO();
    p3d_warm_kernargs<BnSmallArgs>();
    constexpr bool TWO = (MODE == 2 || MODE == 3);
    // CBW channels' worth of summation order: row slot = CBW / 4 neighbouring lanes, RS row slots, chains of 1024 / RS rows.
    // Unsplit, the lanes of a row slot are the block's G channel quads; SPLIT, the block owns ONE quad and they are the P parts of
    // its chain (chain_sum2): 4 rows per thread whatever CBW.
    constexpr int GR = CBW / 4, P = SPLIT ? GR : 1, G = SPLIT ? 1 : GR, RS = 256 / GR, MJ = 1024 / RS / P;
    __shared__ float4 xch[16 * G];
    const int c = xcd_slab((int)blockIdx.x, (int)gridDim.x) * (4 * G) + ((threadIdx.x / P) % G) * 4;
    const int rowslot = threadIdx.x / GR, h = threadIdx.x % P;
    const bool writer = rowslot == 0 && h == 0;
    const int nj = (a.M + RS - 1) / RS;
    const BnChan ch1 = bn_chan_load(a.bn1, c, !a.batch1 || (a.update_moving && writer));
    BnChan ch2 = ch1;
    if (TWO) ch2 = bn_chan_load(a.bn2, c, !a.batch2 || (a.update_moving && writer));
    float4 v1[MJ], v2[MJ];
#pragma unroll
    for (int j = 0; j < MJ; ++j) {
        const int row = rowslot + RS * (h * MJ + j);
        v1[j] = f4(0.f); v2[j] = f4(0.f);
        if (h * MJ + j < nj && row < a.M) {
            v1[j] = ld4(a.y1 + (long long)row * a.ld1 + c);
            if (MODE != 0) v2[j] = ld4(a.y2 + (long long)row * a.ld2 + c);
        }
    }
    int phase = 0;
    float4 mean1 = f4(0.f), var1 = f4(1.f), sc1, sh1, mean2 = f4(0.f), var2 = f4(1.f), sc2 = f4(0.f), sh2 = f4(0.f);
    if (a.batch1) bn_moments<G, P, MJ>(v1, ld4(a.y1 + c), nj, a.M, rowslot, h, xch, phase, mean1, var1);
    bn_coeffs(a.bn1, ch1, c, a.batch1, a.update_moving, a.eps, writer, mean1, var1, sc1, sh1);
    if (TWO) {
        if (a.batch2) bn_moments<G, P, MJ>(v2, ld4(a.y2 + c), nj, a.M, rowslot, h, xch, phase, mean2, var2);
        bn_coeffs(a.bn2, ch2, c, a.batch2, a.update_moving, a.eps, writer, mean2, var2, sc2, sh2);
    }
#pragma unroll
    for (int j = 0; j < MJ; ++j) {
        const int row = rowslot + RS * (h * MJ + j);
        if (h * MJ + j < nj && row < a.M) {
            const float4 v = fma4(sc1, v1[j], sh1);
            float4 z;
            if (MODE == 0) z = relu4(v);
            else if (MODE == 1) z = relu4(add4(v, v2[j]));
            else if (MODE == 2) z = relu4(add4(v, fma4(sc2, v2[j], sh2)));
            else if (MODE == 3) z = add4(relu4(v), relu4(fma4(sc2, v2[j], sh2)));
            else z = add4(v2[j], relu4(v));
            st4(a.z + (long long)row * a.ldz + c, z);
        }
    }
}

template <int MODE, int CBW, bool SPLIT>
__global__ __launch_bounds__(256) void bn_small_bwd_kernel(BnSmallArgs a) {
    P3D_CHAIN_PRIO();
    p3d_warm_kernargs<BnSmallArgs>();
    constexpr bool TWO = (MODE == 2 || MODE == 3);
    // CBW channels' worth of summation order: row slot = CBW / 4 neighbouring lanes, RS row slots, chains of 1024 / RS rows.
    // Unsplit, the lanes of a row slot are the block's G channel quads; SPLIT, the block owns ONE quad and they are the P parts of
    // its chain (chain_sum2): 4 rows per thread whatever CBW.
    constexpr int GR = CBW / 4, P = SPLIT ? GR : 1, G = SPLIT ? 1 : GR, RS = 256 / GR, MJ = 1024 / RS / P;
    __shared__ float4 xch[16 * G];
    const int c = xcd_slab((int)blockIdx.x, (int)gridDim.x) * (4 * G) + ((threadIdx.x / P) % G) * 4;
    const int rowslot = threadIdx.x / GR, h = threadIdx.x % P;
    const bool writer = rowslot == 0 && h == 0;
    const int nj = (a.M + RS - 1) / RS;
    const float4 sc1 = ld4(a.bn1.scale + c), sh1 = ld4(a.bn1.shift + c), m1 = ld4(a.bn1.mean + c), i1 = ld4(a.bn1.invstd + c);
    float4 sc2 = f4(0.f), sh2 = f4(0.f), m2 = f4(0.f), i2 = f4(0.f);
    if (TWO) { sc2 = ld4(a.bn2.scale + c); sh2 = ld4(a.bn2.shift + c); m2 = ld4(a.bn2.mean + c); i2 = ld4(a.bn2.invstd + c); }
    const float4 gam1 = ld4(a.bn1.gamma + c);            // with the data, not behind the reduction (one dependent trip to memory less)
    float4 gam2 = f4(0.f);
    if (TWO) gam2 = ld4(a.bn2.gamma + c);
    float4 g1[MJ], xh1[MJ], g2[MJ], xh2[TWO ? MJ : 1];
    float4 s1 = f4(0.f), sx1 = f4(0.f), s2 = f4(0.f), sx2 = f4(0.f);
#pragma unroll
    for (int j = 0; j < MJ; ++j) {
        const int row = rowslot + RS * (h * MJ + j);
        g1[j] = f4(0.f); xh1[j] = f4(0.f); g2[j] = f4(0.f);
        if (TWO) xh2[TWO ? j : 0] = f4(0.f);
        if (h * MJ + j < nj && row < a.M) {
            const float4 dz = ld4(a.dz + (long long)row * a.lddz + c);
            const float4 y1 = ld4(a.y1 + (long long)row * a.ld1 + c);
            const float4 v1 = fma4(sc1, y1, sh1);
            xh1[j] = mul4(sub4(y1, m1), i1);
            if (MODE == 0) g1[j] = gate4(dz, v1);
            else {
                const float4 y2 = ld4(a.y2 + (long long)row * a.ld2 + c);
                if (MODE == 1) { g1[j] = gate4(dz, add4(v1, y2)); g2[j] = g1[j]; }
                else if (MODE == 4) { g1[j] = gate4(dz, v1); g2[j] = dz; }
                else {
                    const float4 v2 = fma4(sc2, y2, sh2);
                    xh2[TWO ? j : 0] = mul4(sub4(y2, m2), i2);
                    if (MODE == 2) { g1[j] = gate4(dz, add4(v1, v2)); g2[j] = g1[j]; }
                    else { g1[j] = gate4(dz, v1); g2[j] = gate4(dz, v2); }
                }
            }
        }
    }
    const auto live = [&](int j) { return h * MJ + j < nj && rowslot + RS * (h * MJ + j) < a.M; };
    chain_sum2<P, MJ>(s1, sx1, h, [&](int j, float4& s_, float4& q_) { if (live(j)) { s_ = add4(s_, g1[j]); q_ = fma4(g1[j], xh1[j], q_); } });
    if (TWO) chain_sum2<P, MJ>(s2, sx2, h, [&](int j, float4& s_, float4& q_) { if (live(j)) { s_ = add4(s_, g2[j]); q_ = fma4(g2[j], xh2[TWO ? j : 0], q_); } });
    int phase = 0;
    block_sum2<G, P>(s1, sx1, xch, phase++);
    if (TWO) block_sum2<G, P>(s2, sx2, xch, phase++);
    if (writer) {
        st4(a.dbeta1 + c, s1); st4(a.dgamma1 + c, sx1);
        if (TWO) { st4(a.dbeta2 + c, s2); st4(a.dgamma2 + c, sx2); }
    }
    const float invM = 1.f / (float)a.M;
    const float4 k1 = mul4(gam1, i1);
    const float4 c1 = mul4(s1, f4(invM)), cx1 = mul4(sx1, f4(invM));
    float4 k2 = f4(0.f), c2 = f4(0.f), cx2 = f4(0.f);
    if (TWO) { k2 = mul4(gam2, i2); c2 = mul4(s2, f4(invM)); cx2 = mul4(sx2, f4(invM)); }
#pragma unroll
    for (int j = 0; j < MJ; ++j) {
        const int row = rowslot + RS * (h * MJ + j);
        if (h * MJ + j < nj && row < a.M) {
            float4 d = a.batch1 ? mul4(k1, sub4(sub4(g1[j], c1), mul4(xh1[j], cx1))) : mul4(k1, g1[j]);
            st4(a.dy1 + (long long)row * a.lddy1 + c, d);
            if (MODE != 0) {
                float4 e;
                if (TWO) e = a.batch2 ? mul4(k2, sub4(sub4(g2[j], c2), mul4(xh2[TWO ? j : 0], cx2))) : mul4(k2, g2[j]);
                else e = g2[j];
                float* dst = a.dy2 + (long long)row * a.lddy2 + c;
                if (a.acc2) e = add4(e, ld4(dst));
                st4(dst, e);
            }
        }
    }
}

template <int CBW, bool SPLIT>
hipError_t launch_small(const BnSmallArgs& a, bool bwd, hipStream_t s) {
    const dim3 g(a.C / (SPLIT ? 4 : CBW)), b(256);
#define P3D_SM(M_)                                                                          \
    case M_:                                                                                \
        if (bwd) hipLaunchKernelGGL((bn_small_bwd_kernel<M_, CBW, SPLIT>), g, b, 0, s, a);         \
        else hipLaunchKernelGGL((bn_small_fwd_kernel<M_, CBW, SPLIT>), g, b, 0, s, a);             \
        break;
    switch (a.mode) {
        P3D_SM(0) P3D_SM(1) P3D_SM(2) P3D_SM(3) P3D_SM(4)
        default: return hipErrorInvalidValue;
    }
#undef P3D_SM
    return hipGetLastError();
}

}  // namespace

bool p3d_bn_small_ok(long M, int C) { return M <= 1024 && (C % CB) == 0; }

template <int CBW>
hipError_t launch_split(const BnSmallArgs& a, bool bwd, bool split, hipStream_t s) {
    return split && CBW > 4 ? launch_small<CBW, (CBW > 4)>(a, bwd, s) : launch_small<CBW, false>(a, bwd, s);
}

// CBW fixes a channel's summation order (how the rows are dealt to chains and the tree over the chains): 16 for wide tensors, else
// 8, as it has always been, so the results are what they were bit for bit.  What a BLOCK owns is cut narrower: 4 channels, each
// chain split over CBW / 4 lanes (chain_sum2) -- C / 4 blocks, 4 rows per thread, a quarter to an eighth of the bytes per CU.
// Narrow blocks pay only because xcd_slab() keeps the blocks that share a line on one XCD: with slab = block index they were the
// slowest cut (tools/micro/bn_chain per P3D_BN_CB x P3D_BN_SPLIT x P3D_BN_XCD, profiles/r16_bn_chain.log; EXPERIMENTS.md).
static hipError_t dispatch(const BnSmallArgs& a, bool bwd, hipStream_t s) {
    if (!p3d_bn_small_ok(a.M, a.C)) return hipErrorInvalidValue;
#if defined(P3D_TUNING)
    static const hipError_t order = [] {       // P3D_BN_XCD=0: identity slab order (A/B of xcd_slab)
        const char* e = p3d_tune_env("P3D_BN_XCD");
        const int identity = e && atoi(e) == 0;
        return hipMemcpyToSymbol(HIP_SYMBOL(g_bn_slab_identity), &identity, sizeof(int));
    }();
    if (order != hipSuccess) return order;
#endif
    static const int forced = p3d_tune_env("P3D_BN_CB") ? atoi(p3d_tune_env("P3D_BN_CB")) : 0;       // tuning: 4, 8 or 16 channels per slab
    static const int fsplit = p3d_tune_env("P3D_BN_SPLIT") ? atoi(p3d_tune_env("P3D_BN_SPLIT")) : 1; // tuning: 0 = whole slabs per block
    const bool wide = a.C >= 512 && a.C % 16 == 0 && a.mode != 3 && a.mode != 2;
    const bool split = fsplit != 0;
    if (forced == 4) return launch_split<4>(a, bwd, split, s);
    if (forced == 8) return launch_split<8>(a, bwd, split, s);
    if (forced == 16 && a.C % 16 == 0) return launch_split<16>(a, bwd, split, s);
    return wide ? launch_split<16>(a, bwd, split, s) : launch_split<8>(a, bwd, split, s);
}
hipError_t p3d_bn_small_fwd(const BnSmallArgs& a, hipStream_t s) { return dispatch(a, false, s); }
hipError_t p3d_bn_small_bwd(const BnSmallArgs& a, hipStream_t s) { return dispatch(a, true, s); }
