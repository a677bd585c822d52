// Saliency metrics at ground-truth resolution: the evaluation pass of the reference's test.py (test.py:160-183), where
// every 112x112 prediction is resized to the 1080x960 fixation map before it is scored (test.py:166-176).
//
//  * resize_f32_kernel: cv2.resize(float32 map, (W, H), INTER_LINEAR), [n][h][w] -> [n][H][W], up or down.  The coordinate
//    rule of metrics.hip's lin_coef and mapf_kernel's arithmetic (float32 products and sums, horizontal pass then vertical
//    pass), with contraction switched off for the whole file: hipcc fuses a * b + c into one FMA by default, even through
//    the __fmul_rn / __fadd_rn intrinsics of the HIP headers (their bodies are plain operators compiled outside any pragma).
//  * resize_u8_kernel: gen_pred.py:154-168's write-out, cv2.imwrite(cv2.resize(float64(map * 255.), (W, H))): the same
//    coordinates and weights, float64 arithmetic (OpenCV's CV_64F generic path), then imwrite's saturate_cast to uint8.
//  * full_pass_a / full_pass_b / full_sort / full_pass_c / full_borji: CC, SIM, AUC-Judd, AUC-Borji, NSS (and shuffled AUC)
//    of large maps with every map split over many blocks.  Cross-block folds use det_reduce.h (write-through partials, the
//    last arriving block folds them in a fixed order); the only atomics are integer ones (arrival tickets, the AUC-Judd
//    counters).  Results are bit-reproducible.  Arithmetic is float64 on float32 / uint8 inputs, as in metrics.hip.
//
// Inputs of one evaluation (struct P3dFullMaps, p3d_kernels.h), per map b of N pixels:
//    P    the clean saliency map (float32): CC and SIM read it (test.py:172-173);
//    J    = float32(double(P) + jit) when jitter is given: AUC_Judd adds its noise IN PLACE (utils/metrics.py:65 on the
//           copy=False view of :54), so AUC_Borji and NSS of test.py (:175-176) read the jittered map too.  Never stored;
//    D    the density map as float32(v / 255.) of the uint8 resize (mapf_density_kernel); the metrics use v / 255. in
//           double, exactly as test.py's float64 density (dataflow.py:236-238): v = rint(255 * D) recovers the byte;
//    F    the fixation map, uint8 with F / 255. > 0.5 <=> byte >= 128 (dataflow.py:239-241), or float32 > 0.5.
#include "p3d_kernels.h"
#include "det_reduce.h"
#include <math.h>

// no contraction of a * b + c into one rounding anywhere below: the resize must round like OpenCV's generic path and the oracle
#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr int SORT_TPB = 1024;
constexpr int LCAP = 4096;         // AUC-Judd thresholds + counters held in LDS up to this many fixations (32 KB)
constexpr int NA = 11;             // pass A partials per block
constexpr int NB = 8;              // pass B partials per block
constexpr int NS = P3D_FULL_STATS3_PARTS;      // full_stats3 partials per block: min, max, sum, NaN seen
constexpr int NK = P3D_FULL_EXTRA_PARTS;       // full_pass_kl partials per block: KL terms, IG terms, fixated pixels
enum { S_MP, S_MD, S_MNP, S_MXP, S_MND, S_MXD, S_MJ, S_MNJ, S_MXJ, S_NFIX, S_SA, S_SB, S_COUNT };
static_assert(S_COUNT == P3D_FULL_STATS && S_NFIX == P3D_FULL_STAT_NFIX, "p3d_kernels.h names the stats layout");

// fixed-order block reductions through LDS (the tree of metrics.hip); every thread gets the result
__device__ __forceinline__ double block_sum(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int o = TPB / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ double block_min(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int o = TPB / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] = fmin(red[tid], red[tid + o]);
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ double block_max(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int o = TPB / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] = fmax(red[tid], red[tid + o]);
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// ---- resize ---------------------------------------------------------------------------------------------------------
// cv2 (resize.cpp, resizeGeneric_): fx = (float)((dx + 0.5) * scale - 0.5), sx = floor(fx), fx -= sx; clamped to the
// border with weight 0 past it.  scale = src / dst in double.
__device__ __forceinline__ void lin_coef_rn(int d, double scale, int extent, int& s0, int& s1, float& w1) {
    float fx = (float)(((double)d + 0.5) * scale - 0.5);
    int sx = (int)floorf(fx);
    fx -= (float)sx;
    if (sx < 0) { sx = 0; fx = 0.f; }
    if (sx >= extent - 1) { sx = extent - 1; fx = 0.f; }
    s0 = sx; s1 = min(sx + 1, extent - 1); w1 = fx;
}
// The four source taps of destination pixel (y, x) and their weights: one coordinate rule for the float32 and the 8-bit resize.
// src: map m's pixel (y, x) at src[m * map_stride + (y * w + x) * elem_stride] (elem_stride > 1: a channel of a wider
// tensor, e.g. the last frame of every clip in the network's prediction buffer)
struct LinTaps { float p00, p01, p10, p11, wx, wy; };
__device__ __forceinline__ LinTaps lin_taps(const float* f0, int elem_stride, int h, int w, int y, int x, double sy, double sx) {
    int x0, x1, y0, y1; LinTaps t;
    lin_coef_rn(x, sx, w, x0, x1, t.wx);
    lin_coef_rn(y, sy, h, y0, y1, t.wy);
    t.p00 = f0[((size_t)y0 * w + x0) * elem_stride]; t.p01 = f0[((size_t)y0 * w + x1) * elem_stride];
    t.p10 = f0[((size_t)y1 * w + x0) * elem_stride]; t.p11 = f0[((size_t)y1 * w + x1) * elem_stride];
    return t;
}
__global__ __launch_bounds__(TPB) void resize_f32_kernel(const float* src, long long map_stride, int elem_stride, int n, int h, int w,
                                                         float* dst, int H, int W) {
    const double sx = (double)w / W, sy = (double)h / H;
    const long long total = (long long)n * H * W;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long long)gridDim.x * TPB) {
        const int x = (int)(i % W);
        const int y = (int)((i / W) % H);
        const long long m = i / ((long long)W * H);
        const LinTaps t = lin_taps(src + m * map_stride, elem_stride, h, w, y, x, sy, sx);
        const float p00 = t.p00, p01 = t.p01, p10 = t.p10, p11 = t.p11, wx = t.wx, wy = t.wy;
        const float ax = 1.f - wx, ay = 1.f - wy;
        const float r0 = p00 * ax + p01 * wx;
        const float r1 = p10 * ax + p11 * wx;
        dst[i] = r0 * ay + r1 * wy;
    }
}

// ---- 8-bit prediction maps (gen_pred.py:154-168) --------------------------------------------------------------------
// saturate_cast<uchar>(double) as cv2.imwrite's conversion to CV_8U does it on x86: cvRound (round half to even) to int32,
// then clamp to [0, 255].  NaN and a rounded value outside int32 (cvtsd2si's integer-indefinite INT_MIN) give 0.  Spelled
// out rather than left to the hardware's saturating convert, whose out-of-range results differ from x86's.
__device__ __forceinline__ unsigned sat_u8(double v) { return p3d_sat_u8(v); }      // p3d_kernels.h: shared with postprocess.hip
// one pixel: the source is float32(p * scale) widened exactly to double (numpy's float32 product); cv2's CV_64F INTER_LINEAR
// has float32 weights widened to double and double sums, horizontal pass then vertical.  Same size: cv2.resize copies.
__device__ __forceinline__ unsigned resize_u8_px(const float* f0, int elem_stride, int h, int w, int y, int x, double sy, double sx,
                                                 float scale, bool same) {
    if (same) return sat_u8((double)(f0[((size_t)y * w + x) * elem_stride] * scale));
    const LinTaps t = lin_taps(f0, elem_stride, h, w, y, x, sy, sx);
    const double ax = (double)(1.f - t.wx), bx = (double)t.wx, ay = (double)(1.f - t.wy), by = (double)t.wy;
    const double r0 = (double)(t.p00 * scale) * ax + (double)(t.p01 * scale) * bx;
    const double r1 = (double)(t.p10 * scale) * ax + (double)(t.p11 * scale) * bx;
    return sat_u8(r0 * ay + r1 * by);
}
// [n][h][w] float -> [n][H][W] uint8 at dst[off ..): pixel j of this launch is byte off + j of dst (dst 4-byte aligned, off
// arbitrary, so that several launches can pack their maps back to back).  Thread q owns the aligned word of bytes
// 4q .. 4q+3 and stores it whole; only the (at most two) words cut by the launch's ends are stored byte by byte.
// H * W <= INT32_MAX (checked by the callers): in-map offsets are int.
__global__ __launch_bounds__(TPB) void resize_u8_kernel(const float* src, long long map_stride, int elem_stride, int n, int h, int w,
                                                        float scale, unsigned char* dst, long long off, int H, int W) {
    const double sx = (double)w / W, sy = (double)h / H;
    const bool same = h == H && w == W;
    const long long hw = (long long)H * W, end = off + (long long)n * hw;
    const long long q0 = off >> 2, q1 = (end + 3) >> 2;
    for (long long q = q0 + (long long)blockIdx.x * TPB + threadIdx.x; q < q1; q += (long long)gridDim.x * TPB) {
        const long long b0 = max(q << 2, off), b1 = min((q << 2) + 4, end);
        long long m = (b0 - off) / hw;
        int p = (int)(b0 - off - m * hw);
        int y = p / W, x = p - y * W;
        unsigned v[4] = {0u, 0u, 0u, 0u};
        for (long long b = b0; b < b1; ++b) {
            v[b & 3] = resize_u8_px(src + m * map_stride, elem_stride, h, w, y, x, sy, sx, scale, same);
            if (++x == W) { x = 0; if (++y == H) { y = 0; ++m; } }
        }
        if (b1 - b0 == 4) {
            reinterpret_cast<unsigned*>(dst)[q] = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
        } else {
            for (long long b = b0; b < b1; ++b) dst[b] = (unsigned char)v[b & 3];
        }
    }
}

// ---- per-pixel accessors --------------------------------------------------------------------------------------------
__device__ __forceinline__ float jittered(const P3dFullMaps& a, size_t i, float p) {
    return a.jit ? (float)((double)p + a.jit[i]) : p;        // numpy: float32 += float64 -> float64 sum, one rounding
}
__device__ __forceinline__ bool fixated(const P3dFullMaps& a, size_t i) {
    return a.fix_u8 ? ((const unsigned char*)a.fix)[i] >= 128 : ((const float*)a.fix)[i] > 0.5f;
}
__device__ __forceinline__ double density(float q) { return rint((double)q * 255.0) / 255.0; }
__device__ __forceinline__ void block_range(const P3dFullMaps& a, long long& i0, long long& i1) {
    const long long chunk = (a.n_pix + a.nblk - 1) / a.nblk;
    i0 = (long long)blockIdx.x * chunk;
    i1 = min((long long)a.n_pix, i0 + chunk);
}
// fold partials [nblk][stride] of one map in a fixed order: thread t takes blocks t, t + TPB, ..., then the block tree
__device__ __forceinline__ double fold_sum(const double* part, int nblk, int stride, int k, double* red) {
    double v = 0;
    for (int j = threadIdx.x; j < nblk; j += TPB) v += part[(size_t)j * stride + k];
    return block_sum(v, red);
}
__device__ __forceinline__ double fold_min(const double* part, int nblk, int stride, int k, double* red) {
    double v = INFINITY;
    for (int j = threadIdx.x; j < nblk; j += TPB) v = fmin(v, part[(size_t)j * stride + k]);
    return block_min(v, red);
}
__device__ __forceinline__ double fold_max(const double* part, int nblk, int stride, int k, double* red) {
    double v = -INFINITY;
    for (int j = threadIdx.x; j < nblk; j += TPB) v = fmax(v, part[(size_t)j * stride + k]);
    return block_max(v, red);
}

// ---- pass A: sums, minima / maxima, fixation count ------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void full_pass_a(P3dFullMaps a) {
    __shared__ double red[TPB];
    __shared__ int last;
    const int b = blockIdx.y;
    const size_t base = (size_t)b * a.n_pix;
    long long i0, i1;
    block_range(a, i0, i1);
    double sp = 0, sd = 0, sj = 0, nan = 0, nf = 0;
    double mnp = INFINITY, mxp = -INFINITY, mnd = INFINITY, mxd = -INFINITY, mnj = INFINITY, mxj = -INFINITY;
    for (long long i = i0 + threadIdx.x; i < i1; i += TPB) {
        const float p = a.P[base + i];
        const double x = p, j = jittered(a, base + i, p);
        if (x != x || j != j) nan = 1;
        sp += x; mnp = fmin(mnp, x); mxp = fmax(mxp, x);
        sj += j; mnj = fmin(mnj, j); mxj = fmax(mxj, j);
        if (a.D) { const double d = density(a.D[base + i]); sd += d; mnd = fmin(mnd, d); mxd = fmax(mxd, d); }
        nf += fixated(a, base + i) ? 1.0 : 0.0;
    }
    const double v[NA] = {block_sum(sp, red), block_sum(sd, red), block_min(mnp, red), block_max(mxp, red), block_min(mnd, red),
                          block_max(mxd, red), block_sum(sj, red), block_min(mnj, red), block_max(mxj, red), block_max(nan, red),
                          block_sum(nf, red)};
    double* part = a.partA + (size_t)b * a.nblk * NA;
    if (threadIdx.x < NA) p3d_store_wt(part, (size_t)blockIdx.x * NA + threadIdx.x, v[threadIdx.x]);
    if (!p3d_last_block_wt(a.counter + b, a.nblk, &last)) return;
    const double n = (double)a.n_pix;
    const double anynan = fold_max(part, a.nblk, NA, 9, red);
    const double s[S_COUNT] = {fold_sum(part, a.nblk, NA, 0, red) / n, fold_sum(part, a.nblk, NA, 1, red) / n,
                               fold_min(part, a.nblk, NA, 2, red), fold_max(part, a.nblk, NA, 3, red),
                               fold_min(part, a.nblk, NA, 4, red), fold_max(part, a.nblk, NA, 5, red),
                               fold_sum(part, a.nblk, NA, 6, red) / n, fold_min(part, a.nblk, NA, 7, red),
                               fold_max(part, a.nblk, NA, 8, red), fold_sum(part, a.nblk, NA, 10, red), 0.0, 0.0};
    if (threadIdx.x < S_COUNT) {
        const int k = threadIdx.x;
        const bool extremum = k == S_MNP || k == S_MXP || k == S_MND || k == S_MXD || k == S_MNJ || k == S_MXJ;
        a.stats[(size_t)b * S_COUNT + k] = (extremum && anynan > 0.0) ? NAN : s[k];     // np.min / np.max propagate NaN
    }
}

// ---- pass B: centred second moments (CC), range sums (SIM), NSS; the fixated values of J, compacted ------------------
// Slots follow pixel order: block offset = the fixations of the blocks before it (pass A's counts), then wave ballots.
__global__ __launch_bounds__(TPB) void full_pass_b(P3dFullMaps a) {
    __shared__ double red[TPB];
    __shared__ int last, wcnt[TPB / 64];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t base = (size_t)b * a.n_pix;
    const double* st = a.stats + (size_t)b * S_COUNT;
    const double mp = st[S_MP], md = st[S_MD], mj = st[S_MJ];
    const double mnp = st[S_MNP], rp = st[S_MXP] - st[S_MNP], mnd = st[S_MND], rd = st[S_MXD] - st[S_MND];
    const int nfix = a.meta[b * 3 + 0];
    float* fixv = a.fixv + a.meta[b * 3 + 1];
    long long i0, i1;
    block_range(a, i0, i1);
    double before = 0;
    {
        const double* partA = a.partA + (size_t)b * a.nblk * NA;
        for (int j = tid; j < (int)blockIdx.x; j += TPB) before += partA[(size_t)j * NA + 10];
        before = block_sum(before, red);
    }
    int run = (int)before;
    double saa = 0, sbb = 0, sab = 0, sa = 0, sb = 0, var = 0, fs = 0;
    for (long long t0 = i0; t0 < i1; t0 += TPB) {
        const long long i = t0 + tid;
        bool f = false;
        if (i < i1) {
            const float p = a.P[base + i];
            const double x = p, j = jittered(a, base + i, p);
            const double dx = x - mp;
            saa += dx * dx; sa += (x - mnp) / rp;
            if (a.D) {
                const double y = density(a.D[base + i]), dy = y - md;
                sbb += dy * dy; sab += dx * dy; sb += (y - mnd) / rd;
            }
            const double dj = j - mj;
            var += dj * dj;
            f = fixated(a, base + i);
            if (f) fs += dj;
        }
        const unsigned long long m = __ballot(f);
        if (lane == 0) wcnt[wave] = __popcll(m);
        __syncthreads();
        int off = run;
        for (int w = 0; w < wave; ++w) off += wcnt[w];
        if (f) {
            const int slot = off + __popcll(m & ((1ull << lane) - 1ull));
            if (slot < nfix) fixv[slot] = jittered(a, base + i, a.P[base + i]);        // bounded by the caller's count
        }
        for (int w = 0; w < TPB / 64; ++w) run += wcnt[w];
        __syncthreads();
    }
    const double v[NB] = {block_sum(saa, red), block_sum(sbb, red), block_sum(sab, red), block_sum(sa, red),
                          block_sum(sb, red), block_sum(var, red), block_sum(fs, red), 0.0};
    double* part = a.partB + (size_t)b * a.nblk * NB;
    if (tid < NB) p3d_store_wt(part, (size_t)blockIdx.x * NB + tid, v[tid]);
    if (!p3d_last_block_wt(a.counter + b, a.nblk, &last)) return;
    const double Saa = fold_sum(part, a.nblk, NB, 0, red), Sbb = fold_sum(part, a.nblk, NB, 1, red);
    const double Sab = fold_sum(part, a.nblk, NB, 2, red), Sa = fold_sum(part, a.nblk, NB, 3, red);
    const double Sb = fold_sum(part, a.nblk, NB, 4, red), Var = fold_sum(part, a.nblk, NB, 5, red);
    const double Fs = fold_sum(part, a.nblk, NB, 6, red);
    if (tid == 0) {
        a.stats[(size_t)b * S_COUNT + S_SA] = Sa;
        a.stats[(size_t)b * S_COUNT + S_SB] = Sb;
        if (a.out) {
            a.out[b * 5 + 0] = Sab / sqrt(Saa * Sbb);                                  // CC, utils/metrics.py:227-250
            a.out[b * 5 + 4] = (Fs / sqrt(Var / (double)a.n_pix)) / st[S_NFIX];       // NSS, :200-224 (0/0 = NaN: no fixation)
        }
    }
}

// ---- AUC-Judd thresholds: one block per map sorts its fixated values (descending) and clears the counters ----------
__global__ __launch_bounds__(SORT_TPB) void full_sort(P3dFullMaps a) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int nfix = a.meta[b * 3 + 0];
    float* thr = a.fixv + a.meta[b * 3 + 1];
    int* cnt = a.cnt + a.meta[b * 3 + 1] + b;
    int np2 = 1;
    while (np2 < nfix) np2 <<= 1;
    for (int i = nfix + tid; i < np2; i += SORT_TPB) thr[i] = -INFINITY;          // pads sort to the end
    for (int i = tid; i <= np2; i += SORT_TPB) cnt[i] = 0;
    __syncthreads();
    if (nfix < 2) return;
    for (int k = 2; k <= np2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < np2; i += SORT_TPB) {
                const int l = i ^ j;
                if (l > i) {
                    const float x = thr[i], y = thr[l];
                    const bool desc = (i & k) == 0;
                    if (desc ? (x < y) : (x > y)) { thr[i] = y; thr[l] = x; }
                }
            }
            __syncthreads();
        }
}

// ---- pass C: SIM's sum of minima; AUC-Judd's counters (every pixel bisects into the sorted thresholds) ---------------
// thresholds = S at fixated pixels, descending; above[k] = #{S >= thr_k} = prefix sum of the counters; tp[k+1] = (k+1)/n_fix,
// fp[k+1] = (above[k] - k - 1) / (n_pix - n_fix); trapezoids between (0,0) and (1,1) (utils/metrics.py:76-85).
__global__ __launch_bounds__(TPB) void full_pass_c(P3dFullMaps a) {
    __shared__ double red[TPB];
    __shared__ int last, offs[TPB + 1];
    __shared__ float sthr[LCAP];
    __shared__ int cnt[LCAP];
    const int b = blockIdx.y, tid = threadIdx.x;
    const size_t base = (size_t)b * a.n_pix;
    const double* st = a.stats + (size_t)b * S_COUNT;
    const double mnp = st[S_MNP], rp = st[S_MXP] - st[S_MNP], mnd = st[S_MND], rd = st[S_MXD] - st[S_MND];
    const double sa = st[S_SA], sb = st[S_SB];
    const int nfix = a.meta[b * 3 + 0];
    const float* gthr = a.fixv + a.meta[b * 3 + 1];
    int* gcnt = a.cnt + a.meta[b * 3 + 1] + b;
    const bool in_lds = nfix <= LCAP;
    if (in_lds)
        for (int k = tid; k < nfix; k += TPB) { sthr[k] = gthr[k]; cnt[k] = 0; }
    __syncthreads();
    const float* thr = in_lds ? sthr : gthr;
    long long i0, i1;
    block_range(a, i0, i1);
    double acc = 0;
    for (long long i = i0 + tid; i < i1; i += TPB) {
        const float p = a.P[base + i];
        if (a.D) {
            const double x = ((double)p - mnp) / rp / sa, y = (density(a.D[base + i]) - mnd) / rd / sb;
            acc += (x != x) ? x : ((y != y) ? y : fmin(x, y));      // np.minimum propagates NaN from either side
        }
        if (nfix > 0) {
            const float v = jittered(a, base + i, p);
            int lo = 0, hi = nfix;                                   // first threshold index with thr <= v
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (thr[mid] > v) lo = mid + 1; else hi = mid;
            }
            if (lo < nfix) {
                if (in_lds) atomicAdd(&cnt[lo], 1);
                else __hip_atomic_fetch_add(&gcnt[lo], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    __syncthreads();
    if (in_lds)
        for (int k = tid; k < nfix; k += TPB)
            if (cnt[k]) __hip_atomic_fetch_add(&gcnt[k], cnt[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const double sim = block_sum(acc, red);
    double* part = a.partC + (size_t)b * a.nblk;
    if (tid == 0) p3d_store_wt(part, blockIdx.x, sim);
    if (!p3d_last_block_wt(a.counter + b, a.nblk, &last)) return;
    const double Sim = fold_sum(part, a.nblk, 1, 0, red);
    if (tid == 0 && a.out) a.out[b * 5 + 1] = Sim;                   // SIM, utils/metrics.py:258-287
    if (nfix == 0) {
        if (tid == 0 && a.out) a.out[b * 5 + 2] = NAN;               // "no fixation to predict", :56-59
        return;
    }
    // above[k]: prefix sum of the counters, thread chunks then chunk offsets.  The counters were bumped by device-scope
    // atomics of other blocks: every read here is a device-scope load.
    auto ld = [&](int k) { return __hip_atomic_load(&gcnt[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    const int c2 = (nfix + TPB - 1) / TPB;
    const int k0 = min(nfix, tid * c2), k1 = min(nfix, k0 + c2);
    int run = 0;
    for (int k = k0; k < k1; ++k) {
        run += ld(k);
        __hip_atomic_store(&gcnt[k], run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    offs[tid + 1] = run;
    if (tid == 0) offs[0] = 0;
    __syncthreads();
    if (tid == 0) for (int t = 0; t < TPB; ++t) offs[t + 1] += offs[t];
    __syncthreads();
    for (int k = k0; k < k1; ++k) __hip_atomic_store(&gcnt[k], ld(k) + offs[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const double inv_fix = 1.0 / (double)nfix, inv_non = 1.0 / (double)(a.n_pix - nfix);
    double area = 0;
    for (int k = tid; k <= nfix; k += TPB) {
        const double x0 = k == 0 ? 0.0 : (double)(ld(k - 1) - k) * inv_non, y0 = k == 0 ? 0.0 : (double)k * inv_fix;
        const double x1 = k == nfix ? 1.0 : (double)(ld(k) - k - 1) * inv_non, y1 = k == nfix ? 1.0 : (double)(k + 1) * inv_fix;
        area += (x1 - x0) * (y1 + y0) * 0.5;
    }
    area = block_sum(area, red);
    if (tid == 0 && a.out) a.out[b * 5 + 2] = area;                  // AUC_Judd, utils/metrics.py:25-85
}

// ---- AUC-Borji / shuffled AUC: one block per (random split, map) -----------------------------------------------------
// S = J scaled to [0,1] by the map's min / max (pass A); S_fix = the compacted fixated values; S_rand[:, rep] = S at the
// caller's pixel indices r[n_rand][n_rep].  Thresholds arange(0, max(S_fix, S_rand[:, rep]), step) from the top; tp = share
// of S_fix >= thr, fp = #{S_rand >= thr} / n_fix (utils/metrics.py:146-153: also for shuffled AUC's shorter rows, :151-152).
// AUC-Borji: n_rand = n_fix, r = randint(0, n_pix, [n_fix, n_rep]) (:139).  Shuffled AUC: n_rand = min(n_fix, n_other); n_rand_map gives
// every map its own row count (the evaluation pass's shuffled AUC, where n_other differs from clip to clip).
__global__ __launch_bounds__(TPB) void full_borji(P3dFullMaps a, P3dFullBorji r) {
    __shared__ double red[TPB];
    __shared__ int last;
    const int rep = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int nfix = a.meta[b * 3 + 0];
    if (nfix == 0) {                                                 // every block of this map returns here
        if (tid == 0) r.per_rep[(size_t)b * r.n_rep + rep] = NAN;
        if (tid == 0 && rep == 0 && a.out) a.out[b * 5 + 3] = NAN;
        return;
    }
    const int nrand = r.n_rand_map ? r.n_rand_map[b] : (r.n_rand < 0 ? nfix : r.n_rand);
    const size_t base = (size_t)b * a.n_pix;
    const double* st = a.stats + (size_t)b * S_COUNT;
    const double mn = st[S_MNJ], rng = st[S_MXJ] - st[S_MNJ];
    const float* fixv = a.fixv + a.meta[b * 3 + 1];
    const int* idx = r.idx + (size_t)a.meta[b * 3 + 2];
    double top = -INFINITY;
    for (int i = tid; i < nfix; i += TPB) top = fmax(top, ((double)fixv[i] - mn) / rng);
    for (int i = tid; i < nrand; i += TPB) {
        const size_t q = base + idx[(size_t)i * r.n_rep + rep];
        top = fmax(top, ((double)jittered(a, q, a.P[q]) - mn) / rng);
    }
    top = block_max(top, red);
    const int nthr = top > 0.0 ? (int)ceil(top / r.step) : 0;       // len(np.r_[0:top:step])
    double area = 0, px = 0, py = 0;
    for (int k = 0; k < nthr; ++k) {
        const double thr = (double)(nthr - 1 - k) * r.step;
        double ctp = 0, cfp = 0;
        for (int i = tid; i < nfix; i += TPB) ctp += (((double)fixv[i] - mn) / rng >= thr) ? 1.0 : 0.0;
        for (int i = tid; i < nrand; i += TPB) {
            const size_t q = base + idx[(size_t)i * r.n_rep + rep];
            cfp += (((double)jittered(a, q, a.P[q]) - mn) / rng >= thr) ? 1.0 : 0.0;
        }
        ctp = block_sum(ctp, red); cfp = block_sum(cfp, red);
        const double x = cfp / nfix, y = ctp / nfix;
        area += (x - px) * (y + py) * 0.5;
        px = x; py = y;
    }
    area += (1.0 - px) * (1.0 + py) * 0.5;
    if (!a.out) {
        if (tid == 0) r.per_rep[(size_t)b * r.n_rep + rep] = area;
        return;
    }
    if (tid == 0) p3d_store_wt(r.per_rep, (size_t)b * r.n_rep + rep, area);
    if (!p3d_last_block_wt(a.counter + b, r.n_rep, &last)) return;
    const double sum = fold_sum(r.per_rep + (size_t)b * r.n_rep, r.n_rep, 1, 0, red);       // the mean over the splits
    if (tid == 0) a.out[b * 5 + 3] = sum / r.n_rep;
}

// ---- KL divergence and information gain (p3d_set_eval_extra; the law in include/p3d_hip.h) ---------------------------------
// Minimum, maximum and sum of every map, in double on the float32 values: full_pass_a's order (per-lane strided accumulation
// over block_range's chunk, the block tree, the last arriver's fold over blocks) and its NaN rule (a NaN anywhere makes both
// extrema NaN), so that a map gets the bits pass A gives it as P.  The baseline of the information gain, once when it is set.
__global__ __launch_bounds__(TPB) void full_stats3(P3dFullStats3 q) {
    __shared__ double red[TPB];
    __shared__ int last;
    const int b = blockIdx.y;
    const float* m = q.maps + (size_t)b * q.n_pix;
    const long long chunk = (q.n_pix + q.nblk - 1) / q.nblk;
    const long long i0 = (long long)blockIdx.x * chunk, i1 = min((long long)q.n_pix, i0 + chunk);
    double sp = 0, nan = 0, mn = INFINITY, mx = -INFINITY;
    for (long long i = i0 + threadIdx.x; i < i1; i += TPB) {
        const double x = m[i];
        if (x != x) nan = 1;
        sp += x; mn = fmin(mn, x); mx = fmax(mx, x);
    }
    const double v[NS] = {block_min(mn, red), block_max(mx, red), block_sum(sp, red), block_max(nan, red)};
    double* part = q.part + (size_t)b * q.nblk * NS;
    if (threadIdx.x < NS) p3d_store_wt(part, (size_t)blockIdx.x * NS + threadIdx.x, v[threadIdx.x]);
    if (!p3d_last_block_wt(q.counter + b, q.nblk, &last)) return;
    const double anynan = fold_max(part, q.nblk, NS, 3, red);
    const double s[3] = {fold_min(part, q.nblk, NS, 0, red), fold_max(part, q.nblk, NS, 1, red), fold_sum(part, q.nblk, NS, 2, red)};
    if (threadIdx.x < 3) q.out[(size_t)b * 3 + threadIdx.x] = (threadIdx.x < 2 && anynan > 0.0) ? NAN : s[threadIdx.x];
}

// KL = sum q_i log(eps + q_i / (p_i + eps)) and IG = (1 / F) sum over fixated i of (log2(eps + P_i) - log2(eps + B_i)) of every
// map, after pass A.  S1 and S2 are the law's raw sums, not mean * n (S / n * n is not S): pass A's per-block sums still lie in
// partA (no later pass writes it), and every block folds them again in pass A's order -- the double pass A divided by n.  "Any
// element nonzero" is min != 0 or max != 0 (a NaN extremum counts as nonzero, as numpy's any() does).  Op level (e.sstat given):
// the statistics come from full_stats3 and the density is the supplied float32 widened, not density()'s byte.
// F is counted here, in pass A's order (integers: the same double as stats[S_NFIX]).  Each flag is a block-uniform branch: a call
// with KL alone reads neither fixations nor baseline; the baseline's pixel i is e.base[i], one map for all.
__global__ __launch_bounds__(TPB) void full_pass_kl(P3dFullMaps a, P3dFullExtra e) {
    __shared__ double red[TPB];
    __shared__ int last;
    const int b = blockIdx.y;
    const size_t base = (size_t)b * a.n_pix;
    const bool kl = (e.flags & P3D_EXTRA_KLDIV) != 0, ig = (e.flags & P3D_EXTRA_INFO_GAIN) != 0;
    const double n = (double)a.n_pix, eps = 2.2204e-16;
    double mns, mxs, S1, mny = 0, mxy = 0, S2 = 0;
    if (e.sstat) {
        mns = e.sstat[b * 3 + 0]; mxs = e.sstat[b * 3 + 1]; S1 = e.sstat[b * 3 + 2];
        if (kl) { mny = e.ystat[b * 3 + 0]; mxy = e.ystat[b * 3 + 1]; S2 = e.ystat[b * 3 + 2]; }
    } else {
        const double* st = a.stats + (size_t)b * S_COUNT;
        const double* partA = a.partA + (size_t)b * a.nblk * NA;
        mns = st[S_MNP]; mxs = st[S_MXP]; mny = st[S_MND]; mxy = st[S_MXD];
        S1 = fold_sum(partA, a.nblk, NA, 0, red);
        S2 = fold_sum(partA, a.nblk, NA, 1, red);
    }
    const bool any_s = !(mns == 0.0 && mxs == 0.0), any_y = !(mny == 0.0 && mxy == 0.0);
    const double rs = mxs - mns, su = (S1 - n * mns) / rs;
    double mnb = 0, rb = 0, bu = 0;
    if (ig) { mnb = e.bstat[0]; rb = e.bstat[1] - e.bstat[0]; bu = (e.bstat[2] - n * mnb) / rb; }
    long long i0, i1;
    block_range(a, i0, i1);
    double akl = 0, aig = 0, nf = 0;
    for (long long i = i0 + threadIdx.x; i < i1; i += TPB) {
        const double s = a.P[base + i];
        if (kl) {
            const double y = e.sstat ? (double)a.D[base + i] : density(a.D[base + i]);
            const double p = any_s ? s / S1 : s, q = any_y ? y / S2 : y;
            akl += q * log(eps + q / (p + eps));
        }
        if (ig && fixated(a, base + i)) {
            const double Pi = (s - mns) / rs / su, Bi = ((double)e.base[i] - mnb) / rb / bu;
            aig += log2(eps + Pi) - log2(eps + Bi);
            nf += 1.0;
        }
    }
    const double v[NK] = {block_sum(akl, red), block_sum(aig, red), block_sum(nf, red)};
    double* part = e.part + (size_t)b * a.nblk * NK;
    if (threadIdx.x < NK) p3d_store_wt(part, (size_t)blockIdx.x * NK + threadIdx.x, v[threadIdx.x]);
    if (!p3d_last_block_wt(a.counter + b, a.nblk, &last)) return;
    const double KL = fold_sum(part, a.nblk, NK, 0, red), IG = fold_sum(part, a.nblk, NK, 1, red), F = fold_sum(part, a.nblk, NK, 2, red);
    if (threadIdx.x == 0) {
        e.out[b * 2 + 0] = kl ? KL : NAN;
        e.out[b * 2 + 1] = ig ? IG / F : NAN;          // 0 / 0 = NaN: no fixation; a constant or NaN map made every term NaN
    }
}

unsigned grid_for(long long total) { return (unsigned)std::min<long long>((total + TPB - 1) / TPB, 65535); }

}  // namespace

int p3d_full_blocks(long long n_pix) { return (int)std::max<long long>(1, std::min<long long>((n_pix + 4095) / 4096, 1024)); }

hipError_t p3d_resize_f32(const float* src, long long map_stride, int elem_stride, int n, int h, int w, float* dst, int H, int W,
                          hipStream_t s) {
    hipLaunchKernelGGL(resize_f32_kernel, dim3(grid_for((long long)n * H * W)), dim3(TPB), 0, s, src, map_stride, elem_stride, n, h, w,
                       dst, H, W);
    return hipGetLastError();
}
hipError_t p3d_resize_u8(const float* src, long long map_stride, int elem_stride, int n, int h, int w, float scale, unsigned char* dst,
                         long long off, int H, int W, hipStream_t s) {
    const long long words = ((off + (long long)n * H * W + 3) >> 2) - (off >> 2);
    hipLaunchKernelGGL(resize_u8_kernel, dim3(grid_for(words)), dim3(TPB), 0, s, src, map_stride, elem_stride, n, h, w, scale, dst, off,
                       H, W);
    return hipGetLastError();
}
hipError_t p3d_full_moments(const P3dFullMaps& a, hipStream_t s) {
    hipLaunchKernelGGL(full_pass_a, dim3(a.nblk, a.n_maps), dim3(TPB), 0, s, a);
    hipLaunchKernelGGL(full_pass_b, dim3(a.nblk, a.n_maps), dim3(TPB), 0, s, a);
    return hipGetLastError();
}
hipError_t p3d_full_rank(const P3dFullMaps& a, hipStream_t s) {
    hipLaunchKernelGGL(full_sort, dim3(a.n_maps), dim3(SORT_TPB), 0, s, a);
    hipLaunchKernelGGL(full_pass_c, dim3(a.nblk, a.n_maps), dim3(TPB), 0, s, a);
    return hipGetLastError();
}
hipError_t p3d_full_borji(const P3dFullMaps& a, const P3dFullBorji& r, hipStream_t s) {
    hipLaunchKernelGGL(full_borji, dim3(r.n_rep, a.n_maps), dim3(TPB), 0, s, a, r);
    return hipGetLastError();
}
hipError_t p3d_full_stats3(const P3dFullStats3& q, hipStream_t s) {
    if (!q.maps || !q.part || !q.counter || !q.out || q.n_maps < 1 || q.n_maps > 65535 || q.n_pix < 1 || q.nblk != p3d_full_blocks(q.n_pix))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(full_stats3, dim3(q.nblk, q.n_maps), dim3(TPB), 0, s, q);
    return hipGetLastError();
}
hipError_t p3d_full_extra(const P3dFullMaps& a, const P3dFullExtra& e, hipStream_t s) {
    const bool kl = (e.flags & P3D_EXTRA_KLDIV) != 0, ig = (e.flags & P3D_EXTRA_INFO_GAIN) != 0;
    if ((!kl && !ig) || (e.flags & ~(P3D_EXTRA_KLDIV | P3D_EXTRA_INFO_GAIN)) || !a.P || !a.counter || !e.part || !e.out || a.n_maps < 1 ||
        a.n_maps > 65535 || a.n_pix < 1 || a.nblk != p3d_full_blocks(a.n_pix))
        return hipErrorInvalidValue;
    if ((kl && !a.D) || (ig && (!a.fix || !e.base || !e.bstat))) return hipErrorInvalidValue;
    if (e.sstat ? (kl && !e.ystat) : (!a.stats || !a.partA)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(full_pass_kl, dim3(a.nblk, a.n_maps), dim3(TPB), 0, s, a, e);
    return hipGetLastError();
}
