// Per-map saliency losses on gfx950 (p3d_set_loss P3D_LOSS_KLD_CC): w_kld * KL(q || p) + w_cc * (1 - CC) summed over the
// maps, where a map is one [H, W] frame of one clip and p, q are the predicted and ground-truth maps each taken as a
// distribution (reference utils/metrics.py:338-361 KLdiv, eps 2.2204e-16, and :227-250 CC).  Statistics and gradients are
// float64 on float32 inputs (the reference's KLdiv is float32: a deliberate difference).
//
// Three launches, each with P blocks per map, P a function of the map size N alone:
//   map_loss_sums_kernel   S = sum s, Y = sum y                                   -> mstat[m][S, Y]
//   map_loss_terms_kernel  KL, sum g p, and the centred sums A, B, C; CC; the map's loss term, and the total over the maps
//                          (folded in map order) added into *loss_out
//   map_loss_grad_kernel   dlogits = dL/ds * s (1 - s), in double, rounded once
// Blocks of one map combine their partials with det_reduce.h's write-through stores and last-arriver ticket, folded in block
// order; no floating-point atomics.  Every block visits its slice of the map in quads of four elements, as float4 lanes
// when the map can be read that way and element by element otherwise, in the same order on both paths: a map's statistics,
// terms and dlogits depend on its own values and N only -- not on the batch, the map's position in it, or the alignment.
//
// P3D_LOSS_SALIENCY adds w_nss * (-NSS) + w_sim * (1 - SIM) (utils/metrics.py:200-224 and :258-287) and a fixation map, one
// byte per element, in sibling kernels of the same three-stage shape (second half of this file):
//   saliency_loss_sums_kernel   also min and max of s and y, the fixated count F and S_f = sum of s over the fixated elements
//   saliency_loss_terms_kernel  also sum min(p', q') and sum [p' < q'] p'; NSS, SIM and the map's four-term loss
//   saliency_loss_grad_kernel   dlogits with all four terms
#include "p3d_kernels.h"
#include "det_reduce.h"
#include <math.h>

namespace {

constexpr int TPB = 256;
constexpr double KLD_EPS = 2.2204e-16;       // utils/metrics.py:342

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// fixed-order sum of K doubles over the block: lanes by xor-shuffle, then the four waves in order; thread 0 gets the sums
template <int K>
__device__ __forceinline__ void block_fold(double (&v)[K], double (*wsum)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k)
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o);
    __syncthreads();                         // (wsum may still be read from an earlier fold)
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) wsum[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = wsum[0][k] + wsum[1][k] + wsum[2][k] + wsum[3][k];
}

struct Slice {
    long long base;          // first element of the map
    long long q0, q1;        // the block's quads [q0, q1) of the map
    long long m;
};
__device__ __forceinline__ Slice slice_of(const MapLossArgs& a) {
    Slice sl;
    const long long blk = blockIdx.x;
    sl.m = blk / a.blocks;
    const long long b = blk - sl.m * a.blocks;
    const long long quads = (a.N + 3) >> 2, per = (quads + a.blocks - 1) / a.blocks;
    sl.base = sl.m * a.N;
    sl.q0 = b * per;
    sl.q1 = sl.q0 + per < quads ? sl.q0 + per : quads;
    return sl;
}

// The predicted saliency s of a quad and its target: the stored pred on a sigmoid head, the head's own 1/(1+expf(-z)) of
// the raw output otherwise (as sigmoid_ce_kernel).  Returns how many of the four elements lie inside the map.
__device__ __forceinline__ int load_quad(const MapLossArgs& a, long long e, long long left, float (&s)[4], float (&y)[4]) {
    const float* src = a.through_sigmoid ? a.pred : a.logits;
    int n;
    if (a.vec4) {
        const float4 sv = ld4(src + e), yv = ld4(a.target + e);
        s[0] = sv.x; s[1] = sv.y; s[2] = sv.z; s[3] = sv.w;
        y[0] = yv.x; y[1] = yv.y; y[2] = yv.z; y[3] = yv.w;
        n = 4;
    } else {
        n = left < 4 ? (int)left : 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            s[j] = j < n ? src[e + j] : 0.f;
            y[j] = j < n ? a.target[e + j] : 0.f;
        }
    }
    if (!a.through_sigmoid)
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = 1.f / (1.f + expf(-s[j]));
    return n;
}

// p_i and q_i: the map over its sum when the sum is positive, else the map itself (the reference's `if map.any()`)
__device__ __forceinline__ double as_dist(float v, double sum) { return sum > 0.0 ? (double)v / sum : (double)v; }
// g_i = d/dp_i of q_i log(eps + q_i / (p_i + eps))
__device__ __forceinline__ double kl_grad(double p, double q) {
    const double pe = p + KLD_EPS;
    return -(q * q) / (pe * (KLD_EPS * pe + q));
}

__global__ __launch_bounds__(TPB) void map_loss_sums_kernel(MapLossArgs a) {
    P3D_CHAIN_PRIO();
    __shared__ double wsum[4][2];
    __shared__ int last_flag;
    const Slice sl = slice_of(a);
    double v[2] = {0.0, 0.0};
    for (long long q = sl.q0 + threadIdx.x; q < sl.q1; q += TPB) {
        float s[4], y[4];
        const int n = load_quad(a, sl.base + 4 * q, a.N - 4 * q, s, y);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < n) { v[0] += s[j]; v[1] += y[j]; }
    }
    block_fold<2>(v, wsum);
    double* part = a.part + sl.m * a.blocks * 2;
    const long long b = blockIdx.x - sl.m * a.blocks;
    if (threadIdx.x == 0) { p3d_store_wt(part, b * 2, v[0]); p3d_store_wt(part, b * 2 + 1, v[1]); }
    if (!p3d_last_block_wt(a.cnt + sl.m, a.blocks, &last_flag)) return;
    double t[2] = {0.0, 0.0};
    if (threadIdx.x < a.blocks) { t[0] = part[threadIdx.x * 2]; t[1] = part[threadIdx.x * 2 + 1]; }
    block_fold<2>(t, wsum);
    if (threadIdx.x == 0) { a.mstat[sl.m * P3D_MAP_STATS + 0] = t[0]; a.mstat[sl.m * P3D_MAP_STATS + 1] = t[1]; }
}

__global__ __launch_bounds__(TPB) void map_loss_terms_kernel(MapLossArgs a) {
    P3D_CHAIN_PRIO();
    __shared__ double wsum[4][5];
    __shared__ double red[TPB];
    __shared__ int last_flag;
    const Slice sl = slice_of(a);
    double* ms = a.mstat + sl.m * P3D_MAP_STATS;
    const double S = ms[0], Y = ms[1], sbar = S / (double)a.N, ybar = Y / (double)a.N;
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};      // KL, sum g p, A, B, C
    for (long long q = sl.q0 + threadIdx.x; q < sl.q1; q += TPB) {
        float s[4], y[4];
        const int n = load_quad(a, sl.base + 4 * q, a.N - 4 * q, s, y);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < n) {
                const double p = as_dist(s[j], S), qq = as_dist(y[j], Y);
                v[0] += qq * log(KLD_EPS + qq / (p + KLD_EPS));
                v[1] += kl_grad(p, qq) * p;
                const double ds = (double)s[j] - sbar, dy = (double)y[j] - ybar;
                v[2] += ds * ds; v[3] += dy * dy; v[4] += ds * dy;
            }
    }
    block_fold<5>(v, wsum);
    double* part = a.part + sl.m * a.blocks * 5;
    const long long b = blockIdx.x - sl.m * a.blocks;
    if (threadIdx.x == 0)
        for (int k = 0; k < 5; ++k) p3d_store_wt(part, b * 5 + k, v[k]);
    if (!p3d_last_block_wt(a.cnt + sl.m, a.blocks, &last_flag)) return;
    // the map's last block: its statistics, CC and loss term
    double t[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (threadIdx.x < a.blocks)
        for (int k = 0; k < 5; ++k) t[k] = part[threadIdx.x * 5 + k];
    block_fold<5>(t, wsum);
    if (threadIdx.x == 0) {
        const double A = t[2], B = t[3], C = t[4];
        const bool defined = A > 0.0 && B > 0.0;         // else CC is undefined (NaN) and the map adds 0 to the CC term
        const double cc = defined ? C / (sqrt(A) * sqrt(B)) : __longlong_as_double(0x7ff8000000000000ll);
        const double lm = (double)a.kld_weight * t[0] + (defined ? (double)a.cc_weight * (1.0 - cc) : 0.0);
        p3d_store_wt(ms, 2, t[0]); p3d_store_wt(ms, 3, cc); p3d_store_wt(ms, 4, t[1]);
        p3d_store_wt(ms, 5, A); p3d_store_wt(ms, 6, B); p3d_store_wt(ms, 7, C); p3d_store_wt(ms, 8, lm);
    }
    // the last map: the total, in map order (each thread folds a run of consecutive maps, then the runs in order)
    if (!p3d_last_block_wt(a.cnt + a.maps, (unsigned)a.maps, &last_flag)) return;
    const long long run = (a.maps + TPB - 1) / TPB, m0 = threadIdx.x * run;
    double acc = 0.0;
    for (long long m = m0; m < m0 + run && m < a.maps; ++m) acc += a.mstat[m * P3D_MAP_STATS + 8];
    red[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int i = 0; i < TPB; ++i) total += red[i];
        *a.loss_out += total;
    }
}

__global__ __launch_bounds__(TPB) void map_loss_grad_kernel(MapLossArgs a) {
    P3D_CHAIN_PRIO();
    const Slice sl = slice_of(a);
    const double* ms = a.mstat + sl.m * P3D_MAP_STATS;
    const double S = ms[0], Y = ms[1], cc = ms[3], gp = ms[4], A = ms[5], B = ms[6];
    const double sbar = S / (double)a.N, ybar = Y / (double)a.N;
    const bool defined = A > 0.0 && B > 0.0;
    const double rab = defined ? 1.0 / (sqrt(A) * sqrt(B)) : 0.0, cca = defined ? cc / A : 0.0;
    const double wk = a.kld_weight, wc = a.cc_weight;
    for (long long q = sl.q0 + threadIdx.x; q < sl.q1; q += TPB) {
        float s[4], y[4], d[4];
        const long long e = sl.base + 4 * q;
        const int n = load_quad(a, e, a.N - 4 * q, s, y);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double p = as_dist(s[j], S), qq = as_dist(y[j], Y), g = kl_grad(p, qq);
            const double dkl = S > 0.0 ? (g - gp) / S : g;
            const double dcc = ((double)y[j] - ybar) * rab - cca * ((double)s[j] - sbar);
            d[j] = (float)((wk * dkl - wc * dcc) * ((double)s[j] * (1.0 - (double)s[j])));
        }
        if (a.vec4) st4(a.dlogits + e, make_float4(d[0], d[1], d[2], d[3]));
        else
            for (int j = 0; j < n; ++j) a.dlogits[e + j] = d[j];
    }
}


// ---- P3D_LOSS_SALIENCY: the three launches above with the NSS and SIM terms, as sibling kernels (the launches of
// P3D_LOSS_KLD_CC stay as they are).  The KL and CC statistics are accumulated by the same expressions in the same order.
constexpr double DBL_INF = __builtin_huge_val();

// which of a quad's elements are fixated (byte >= 128): one 32-bit load on the float4 path, else byte by byte, same order
__device__ __forceinline__ void load_fix(const SaliencyLossArgs& a, long long e, int n, bool (&f)[4]) {
    if (!a.use_fix) {
#pragma unroll
        for (int j = 0; j < 4; ++j) f[j] = false;
    } else if (a.m.vec4) {
        const unsigned w = *reinterpret_cast<const unsigned*>(a.fix + e);
#pragma unroll
        for (int j = 0; j < 4; ++j) f[j] = ((w >> (8 * j + 7)) & 1u) != 0;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) f[j] = j < n && a.fix[e + j] >= 128;
    }
}

// min of v[0], v[2] and max of v[1], v[3] over the block (order does not matter for either); thread 0 gets them
__device__ __forceinline__ void block_minmax(double (&v)[4], double (*wmm)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
        for (int o = 32; o > 0; o >>= 1) {
            const double w = __shfl_xor(v[k], o);
            v[k] = (k & 1) ? fmax(v[k], w) : fmin(v[k], w);
        }
    __syncthreads();
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < 4; ++k) wmm[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < 4; ++k)
            v[k] = (k & 1) ? fmax(fmax(wmm[0][k], wmm[1][k]), fmax(wmm[2][k], wmm[3][k]))
                           : fmin(fmin(wmm[0][k], wmm[1][k]), fmin(wmm[2][k], wmm[3][k]));
}

// what the stages after the first derive from a map's statistics
struct SalMap {
    double S, Y, sbar, ybar;
    double lo_s, lo_y, Ds, Dy;       // p'_i = (s_i - lo_s) / Ds, Ds = (hi_s - lo_s) U = S - N lo_s; q' likewise
    double F, Sf;
    bool sim_defined;
};
__device__ __forceinline__ SalMap sal_map(const SaliencyLossArgs& a, long long m) {
    const double* ms = a.m.mstat + m * P3D_MAP_STATS;
    const double* xs = a.xstat + m * P3D_SAL_STATS;
    SalMap r;
    const double N = (double)a.m.N;
    r.S = ms[0]; r.Y = ms[1]; r.sbar = r.S / N; r.ybar = r.Y / N;
    r.lo_s = xs[0]; r.lo_y = xs[2];
    r.sim_defined = xs[1] > xs[0] && xs[3] > xs[2];
    r.Ds = r.S - N * r.lo_s; r.Dy = r.Y - N * r.lo_y;
    r.F = xs[4]; r.Sf = xs[5];
    return r;
}

__global__ __launch_bounds__(TPB) void saliency_loss_sums_kernel(SaliencyLossArgs a) {
    P3D_CHAIN_PRIO();
    __shared__ double wsum[4][4];
    __shared__ double wmm[4][4];
    __shared__ int last_flag;
    const Slice sl = slice_of(a.m);
    double v[4] = {0.0, 0.0, 0.0, 0.0};                      // S, Y, F, S_f
    double mm[4] = {DBL_INF, -DBL_INF, DBL_INF, -DBL_INF};    // min s, max s, min y, max y
    for (long long q = sl.q0 + threadIdx.x; q < sl.q1; q += TPB) {
        float s[4], y[4];
        bool f[4];
        const long long e = sl.base + 4 * q;
        const int n = load_quad(a.m, e, a.m.N - 4 * q, s, y);
        load_fix(a, e, n, f);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < n) {
                v[0] += s[j]; v[1] += y[j];
                if (f[j]) { v[2] += 1.0; v[3] += s[j]; }
                mm[0] = fmin(mm[0], (double)s[j]); mm[1] = fmax(mm[1], (double)s[j]);
                mm[2] = fmin(mm[2], (double)y[j]); mm[3] = fmax(mm[3], (double)y[j]);
            }
    }
    block_fold<4>(v, wsum);
    block_minmax(mm, wmm);
    double* part = a.m.part + sl.m * a.m.blocks * P3D_SAL_PARTS;
    const long long b = blockIdx.x - sl.m * a.m.blocks;
    if (threadIdx.x == 0)
        for (int k = 0; k < 4; ++k) { p3d_store_wt(part, b * P3D_SAL_PARTS + k, v[k]); p3d_store_wt(part, b * P3D_SAL_PARTS + 4 + k, mm[k]); }
    if (!p3d_last_block_wt(a.m.cnt + sl.m, a.m.blocks, &last_flag)) return;
    double t[4] = {0.0, 0.0, 0.0, 0.0};
    double tm[4] = {DBL_INF, -DBL_INF, DBL_INF, -DBL_INF};
    if (threadIdx.x < a.m.blocks)
        for (int k = 0; k < 4; ++k) { t[k] = part[threadIdx.x * P3D_SAL_PARTS + k]; tm[k] = part[threadIdx.x * P3D_SAL_PARTS + 4 + k]; }
    block_fold<4>(t, wsum);
    block_minmax(tm, wmm);
    if (threadIdx.x == 0) {
        double* ms = a.m.mstat + sl.m * P3D_MAP_STATS;
        double* xs = a.xstat + sl.m * P3D_SAL_STATS;
        ms[0] = t[0]; ms[1] = t[1];
        xs[0] = tm[0]; xs[1] = tm[1]; xs[2] = tm[2]; xs[3] = tm[3]; xs[4] = t[2]; xs[5] = t[3];
    }
}

__global__ __launch_bounds__(TPB) void saliency_loss_terms_kernel(SaliencyLossArgs a) {
    P3D_CHAIN_PRIO();
    __shared__ double wsum[4][7];
    __shared__ double red[TPB];
    __shared__ int last_flag;
    const Slice sl = slice_of(a.m);
    const SalMap mp = sal_map(a, sl.m);
    const double S = mp.S, Y = mp.Y, sbar = mp.sbar, ybar = mp.ybar;
    double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // KL, sum g p, A, B, C, sum min(p', q'), sum [p' < q'] p'
    for (long long q = sl.q0 + threadIdx.x; q < sl.q1; q += TPB) {
        float s[4], y[4];
        const int n = load_quad(a.m, sl.base + 4 * q, a.m.N - 4 * q, s, y);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < n) {
                const double p = as_dist(s[j], S), qq = as_dist(y[j], Y);
                v[0] += qq * log(KLD_EPS + qq / (p + KLD_EPS));
                v[1] += kl_grad(p, qq) * p;
                const double ds = (double)s[j] - sbar, dy = (double)y[j] - ybar;
                v[2] += ds * ds; v[3] += dy * dy; v[4] += ds * dy;
                if (mp.sim_defined) {
                    const double pp = ((double)s[j] - mp.lo_s) / mp.Ds, qp = ((double)y[j] - mp.lo_y) / mp.Dy;
                    const bool below = pp < qp;
                    v[5] += below ? pp : qp;
                    if (below) v[6] += pp;
                }
            }
    }
    block_fold<7>(v, wsum);
    double* part = a.m.part + sl.m * a.m.blocks * P3D_SAL_PARTS;
    const long long b = blockIdx.x - sl.m * a.m.blocks;
    if (threadIdx.x == 0)
        for (int k = 0; k < 7; ++k) p3d_store_wt(part, b * P3D_SAL_PARTS + k, v[k]);
    if (!p3d_last_block_wt(a.m.cnt + sl.m, a.m.blocks, &last_flag)) return;
    // the map's last block: its statistics, CC, NSS, SIM and loss term
    double t[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (threadIdx.x < a.m.blocks)
        for (int k = 0; k < 7; ++k) t[k] = part[threadIdx.x * P3D_SAL_PARTS + k];
    block_fold<7>(t, wsum);
    if (threadIdx.x == 0) {
        double* ms = a.m.mstat + sl.m * P3D_MAP_STATS;
        double* xs = a.xstat + sl.m * P3D_SAL_STATS;
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        const double A = t[2], B = t[3], C = t[4];
        const bool defined = A > 0.0 && B > 0.0;         // as map_loss_terms_kernel
        const double cc = defined ? C / (sqrt(A) * sqrt(B)) : nan;
        double lm = (double)a.m.kld_weight * t[0] + (defined ? (double)a.m.cc_weight * (1.0 - cc) : 0.0);
        // NSS needs a fixation and a spread of s; SIM a spread of both maps: else NaN, and the map adds 0 to that term
        const bool nss_defined = a.use_fix && mp.F > 0.0 && A > 0.0;
        const double nss = nss_defined ? (mp.Sf / mp.F - sbar) / sqrt(A / (double)a.m.N) : nan;
        const double sim = mp.sim_defined ? t[5] : nan;
        if (a.nss_weight > 0.f && nss_defined) lm -= (double)a.nss_weight * nss;
        if (a.sim_weight > 0.f && mp.sim_defined) lm += (double)a.sim_weight * (1.0 - sim);
        p3d_store_wt(ms, 2, t[0]); p3d_store_wt(ms, 3, cc); p3d_store_wt(ms, 4, t[1]);
        p3d_store_wt(ms, 5, A); p3d_store_wt(ms, 6, B); p3d_store_wt(ms, 7, C); p3d_store_wt(ms, 8, lm);
        p3d_store_wt(xs, 6, nss); p3d_store_wt(xs, 7, sim); p3d_store_wt(xs, 8, t[6]);
    }
    // the last map: the total, in map order (as map_loss_terms_kernel)
    if (!p3d_last_block_wt(a.m.cnt + a.m.maps, (unsigned)a.m.maps, &last_flag)) return;
    const long long run = (a.m.maps + TPB - 1) / TPB, m0 = threadIdx.x * run;
    double acc = 0.0;
    for (long long m = m0; m < m0 + run && m < a.m.maps; ++m) acc += a.m.mstat[m * P3D_MAP_STATS + 8];
    red[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int i = 0; i < TPB; ++i) total += red[i];
        *a.m.loss_out += total;
    }
}

__global__ __launch_bounds__(TPB) void saliency_loss_grad_kernel(SaliencyLossArgs a) {
    P3D_CHAIN_PRIO();
    const Slice sl = slice_of(a.m);
    const SalMap mp = sal_map(a, sl.m);
    const double* ms = a.m.mstat + sl.m * P3D_MAP_STATS;
    const double* xs = a.xstat + sl.m * P3D_SAL_STATS;
    const double S = mp.S, Y = mp.Y, cc = ms[3], gp = ms[4], A = ms[5], B = ms[6];
    const double sbar = mp.sbar, ybar = mp.ybar;
    const bool defined = A > 0.0 && B > 0.0;
    const double rab = defined ? 1.0 / (sqrt(A) * sqrt(B)) : 0.0, cca = defined ? cc / A : 0.0;
    const double wk = a.m.kld_weight, wc = a.m.cc_weight, wn = a.nss_weight, ws = a.sim_weight;
    // dNSS/ds_i = (f_i / F - 1 / N) / sigma - NSS (s_i - sbar) / A;  dSIM/ds_i = ([p'_i < q'_i] - G) / Ds, the range held fixed
    const bool with_nss = wn > 0.0 && a.use_fix && mp.F > 0.0 && A > 0.0, with_sim = ws > 0.0 && mp.sim_defined;
    const double rsig = with_nss ? 1.0 / sqrt(A / (double)a.m.N) : 0.0, rF = with_nss ? 1.0 / mp.F : 0.0;
    const double rN = 1.0 / (double)a.m.N, nssa = with_nss ? xs[6] / A : 0.0, G = xs[8];
    for (long long q = sl.q0 + threadIdx.x; q < sl.q1; q += TPB) {
        float s[4], y[4], d[4];
        bool f[4];
        const long long e = sl.base + 4 * q;
        const int n = load_quad(a.m, e, a.m.N - 4 * q, s, y);
        if (with_nss) load_fix(a, e, n, f);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double p = as_dist(s[j], S), qq = as_dist(y[j], Y), g = kl_grad(p, qq);
            const double dkl = S > 0.0 ? (g - gp) / S : g;
            const double dcc = ((double)y[j] - ybar) * rab - cca * ((double)s[j] - sbar);
            double dl = wk * dkl - wc * dcc;
            if (with_nss) dl -= wn * (((f[j] ? rF : 0.0) - rN) * rsig - nssa * ((double)s[j] - sbar));
            if (with_sim) {
                const double pp = ((double)s[j] - mp.lo_s) / mp.Ds, qp = ((double)y[j] - mp.lo_y) / mp.Dy;
                dl -= ws * (((pp < qp ? 1.0 : 0.0) - G) / mp.Ds);
            }
            d[j] = (float)(dl * ((double)s[j] * (1.0 - (double)s[j])));
        }
        if (a.m.vec4) st4(a.m.dlogits + e, make_float4(d[0], d[1], d[2], d[3]));
        else
            for (int j = 0; j < n; ++j) a.m.dlogits[e + j] = d[j];
    }
}

}  // namespace

int p3d_map_loss_blocks(long long map_elems) {
    const long long p = (map_elems + P3D_MAP_LOSS_ELEMS_PER_BLOCK - 1) / P3D_MAP_LOSS_ELEMS_PER_BLOCK;
    return (int)(p < 1 ? 1 : (p > 256 ? 256 : p));
}

void p3d_map_loss_scratch(long long maps, long long map_elems, size_t* doubles, size_t* counters) {
    // mstat, then the partials (five per block: the terms launch; the sums launch uses the first two of each)
    *doubles = (size_t)maps * P3D_MAP_STATS + (size_t)maps * p3d_map_loss_blocks(map_elems) * 5;
    *counters = (size_t)maps + 1;        // one per map, one for the total
}

MapLossArgs p3d_map_loss_args(const float* logits, const float* pred, const float* target, long long maps, long long map_elems,
                              int through_sigmoid, float kld_weight, float cc_weight, double* loss_out, float* dlogits,
                              double* scratch, unsigned* counters) {
    MapLossArgs a;
    a.logits = logits; a.pred = pred; a.target = target; a.dlogits = dlogits; a.loss_out = loss_out;
    a.maps = maps; a.N = map_elems; a.blocks = p3d_map_loss_blocks(map_elems);
    a.through_sigmoid = through_sigmoid ? 1 : 0;
    a.kld_weight = kld_weight; a.cc_weight = cc_weight;
    a.mstat = scratch; a.part = scratch + (size_t)maps * P3D_MAP_STATS; a.cnt = counters;
    const uintptr_t src = reinterpret_cast<uintptr_t>(a.through_sigmoid ? pred : logits);
    a.vec4 = (map_elems & 3) == 0 && ((src | reinterpret_cast<uintptr_t>(target) | reinterpret_cast<uintptr_t>(dlogits)) & 15) == 0;
    return a;
}

hipError_t p3d_map_loss_launch(int stage, const MapLossArgs& a, hipStream_t s) {
    if (a.maps < 1 || a.N < 1 || stage < 0 || stage > 2) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(a.maps * a.blocks));
    if (stage == 0) hipLaunchKernelGGL(map_loss_sums_kernel, grid, dim3(TPB), 0, s, a);
    else if (stage == 1) hipLaunchKernelGGL(map_loss_terms_kernel, grid, dim3(TPB), 0, s, a);
    else hipLaunchKernelGGL(map_loss_grad_kernel, grid, dim3(TPB), 0, s, a);
    return hipGetLastError();
}

void p3d_saliency_loss_scratch(long long maps, long long map_elems, size_t* doubles, size_t* counters) {
    // mstat, xstat, then the partials (P3D_SAL_PARTS per block)
    *doubles = (size_t)maps * (P3D_MAP_STATS + P3D_SAL_STATS) + (size_t)maps * p3d_map_loss_blocks(map_elems) * P3D_SAL_PARTS;
    *counters = (size_t)maps + 1;
}

SaliencyLossArgs p3d_saliency_loss_args(const float* logits, const float* pred, const float* target, const unsigned char* fix,
                                        long long maps, long long map_elems, int through_sigmoid, float kld_weight, float cc_weight,
                                        float nss_weight, float sim_weight, double* loss_out, float* dlogits, double* scratch,
                                        unsigned* counters) {
    SaliencyLossArgs a;
    a.m = p3d_map_loss_args(logits, pred, target, maps, map_elems, through_sigmoid, kld_weight, cc_weight, loss_out, dlogits, scratch,
                            counters);
    a.xstat = scratch + (size_t)maps * P3D_MAP_STATS;
    a.m.part = a.xstat + (size_t)maps * P3D_SAL_STATS;
    a.nss_weight = nss_weight; a.sim_weight = sim_weight;
    a.use_fix = nss_weight > 0.f ? 1 : 0;          // with no NSS term the fixations are not read
    a.fix = a.use_fix ? fix : nullptr;
    if (a.use_fix && (reinterpret_cast<uintptr_t>(fix) & 3)) a.m.vec4 = 0;
    return a;
}

hipError_t p3d_saliency_loss_launch(int stage, const SaliencyLossArgs& a, hipStream_t s) {
    if (a.m.maps < 1 || a.m.N < 1 || stage < 0 || stage > 2 || (a.use_fix && !a.fix)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(a.m.maps * a.m.blocks));
    if (stage == 0) hipLaunchKernelGGL(saliency_loss_sums_kernel, grid, dim3(TPB), 0, s, a);
    else if (stage == 1) hipLaunchKernelGGL(saliency_loss_terms_kernel, grid, dim3(TPB), 0, s, a);
    else hipLaunchKernelGGL(saliency_loss_grad_kernel, grid, dim3(TPB), 0, s, a);
    return hipGetLastError();
}
