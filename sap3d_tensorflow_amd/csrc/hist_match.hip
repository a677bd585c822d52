// Histogram matching of output maps (p3d_set_hist_match, p3d_match_hist; HistArgs in p3d_kernels.h, the law in include/p3d_hip.h):
// the reference's utils/metric_utils.py:56-84 match_hist on exposure.cumulative_distribution tables, i.e. np.histogram and np.interp,
// in float64 on float32 maps, every operation rounded on its own.
//
//  * HIST_MINMAX: postprocess.hip's minmax_kernel (float32 min / max are exact) into buffers of this stage's own.
//  * hist_count_kernel<KIND>: grid (nblk, n).  A lane takes one pixel per pass, finds its bin by the law (one multiply, then
//    the two fix-ups against the edges) and counts it in LDS.  Saliency maps are extremely skewed -- half of a u^8 map sits in
//    bin 0 of 256 -- and a plain one-counter-per-bin LDS histogram serialises on that bin, so (a) every wave owns a private
//    copy of the counters and (b) before the add, up to three candidate bins of a wave are each counted with one ballot: the
//    lanes of a candidate that holds four lanes or more retire with ONE add of their number.  What is left adds 1 per lane.
//    Counts are integers: the order of the adds cannot show.  The copies are folded and flushed to the map's global integer
//    table (zeroed by the launcher in stream order); the last arriving block of the map (det_reduce.h's ticket) turns the table
//    into count / centre / cdf and, when the target's table is given, the nb values of `new`.
//    KIND HIST_DENSITY reads evaluation's density map: the float32 (b / 255.) of a resized byte b, taken back to the double
//    b / 255. that the metrics use (metrics_full.hip's density()).
//  * hist_remap_kernel: centre, new and the nb - 1 slopes (new[j+1] - new[j]) / (centre[j+1] - centre[j]) of one map staged in
//    LDS (the slope is the law's own quotient, computed once per interval instead of once per pixel: the same bits).  One lane
//    per pixel; whole 16-byte words where source and destination are aligned alike.  The interval is guessed by one multiply
//    and then corrected against the staged centres until it is the largest j with centre[j] <= x: the guess is never trusted.
//    Every element is written by exactly one lane, in place or not.
#include "p3d_kernels.h"
#include "det_reduce.h"
#include "../../include/p3d_hip.h"
#include <math.h>
#include <algorithm>

// every product, quotient and sum below rounds on its own (the header's law): hipcc would otherwise fuse a * b + c
#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr int NBMAX = P3D_HIST_BINS_CAP;
static_assert(P3D_HIST_BINS_CAP == P3D_HIST_MAX_BINS, "the ABI names the kernels' bound");

template <int KIND>
__device__ __forceinline__ double hist_value(float q) {
    return KIND == HIST_DENSITY ? rint((double)q * 255.0) / 255.0 : (double)q;
}

// np.interp(x, xp, fp) over n entries, xp non-decreasing (the header's interp)
__device__ __forceinline__ double interp_law(double x, const double* __restrict__ xp, const double* __restrict__ fp, int n) {
    if (x < xp[0]) return fp[0];
    if (x >= xp[n - 1]) return fp[n - 1];
    int lo = 0, hi = n - 1;                                // xp[lo] <= x < xp[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (xp[mid] <= x) lo = mid; else hi = mid;
    }
    if (x == xp[lo]) return fp[lo];
    return ((fp[lo + 1] - fp[lo]) / (xp[lo + 1] - xp[lo])) * (x - xp[lo]) + fp[lo];
}

__device__ __forceinline__ void table_add(int* cnt, int k, int v) { __hip_atomic_fetch_add(&cnt[k], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// grid (nblk, n): block j of map m counts pixels [j * chunk, (j + 1) * chunk)
template <int KIND>
__global__ __launch_bounds__(TPB) void hist_count_kernel(HistArgs a) {
    __shared__ int cnt[WAVES * NBMAX];
    __shared__ long long offs[TPB + 1];
    __shared__ int last;
    const int m = blockIdx.y, tid = threadIdx.x, lane = tid & 63, nb = a.nb;
    const int n_pix = a.H * a.W;
    const float* p = a.maps + (size_t)m * n_pix;
    double mn = hist_value<KIND>(a.mnmx[m * 2]), mx = hist_value<KIND>(a.mnmx[m * 2 + 1]);
    if (mn == mx) { mn = mn - 0.5; mx = mx + 0.5; }
    const double step = (mx - mn) / (double)nb, norm = (double)nb / (mx - mn);
    auto edge = [&](int k) { return k == nb ? mx : mn + (double)k * step; };
    for (int k = tid; k < WAVES * nb; k += TPB) cnt[k] = 0;
    __syncthreads();
    const int chunk = (n_pix + a.nblk - 1) / a.nblk;
    const int i0 = (int)min((long long)blockIdx.x * chunk, (long long)n_pix), i1 = (int)min((long long)i0 + chunk, (long long)n_pix);
    for (int at = i0; at < i1; at += TPB) {                // a wave-uniform trip count: the ballots below need every lane
        const int i = at + tid;
        int b = -1;
        if (i < i1) {
            const double v = hist_value<KIND>(p[i]);
            const double g = (v - mn) * norm;
            b = g >= 0.0 ? (g < (double)nb ? (int)g : nb) : 0;        // (int)g of the law; NaN and inf (not pinned) stay in range
            if (b == nb) b = nb - 1;
            if (v < edge(b)) b -= 1;
            else if (v >= edge(b + 1) && b != nb - 1) b += 1;
            b = max(0, min(b, nb - 1));                    // the law never leaves [0, nb) on finite maps; NaN must not either
        }
        unsigned long long cand = __ballot(b >= 0);
        for (int round = 0; round < 3 && cand; ++round) {
            const int lead = __shfl(b, __ffsll((long long)cand) - 1);
            const unsigned long long same = __ballot(b == lead);
            if (__popcll(same) >= 4) {
                if (lane == __ffsll((long long)same) - 1) atomicAdd(&cnt[(tid >> 6) * nb + lead], __popcll(same));
                if (b == lead) b = -1;
            }
            cand &= ~same;
        }
        if (b >= 0) atomicAdd(&cnt[(tid >> 6) * nb + b], 1);
    }
    __syncthreads();
    int* table = a.cnt + (size_t)m * nb;
    for (int k = tid; k < nb; k += TPB) {
        int tot = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) tot += cnt[w * nb + k];
        if (tot) table_add(table, k, tot);
    }
    if (!p3d_last_block_wt(a.counter + m, a.nblk, &last)) return;
    // the table was bumped by device-scope atomics of other blocks: every read of it here is a device-scope load
    const int c2 = (nb + TPB - 1) / TPB;
    const int k0 = min(nb, tid * c2), k1 = min(nb, k0 + c2);
    long long run = 0;
    for (int k = k0; k < k1; ++k) {
        const int c = __hip_atomic_load(&table[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        cnt[k] = c;
        run += c;
    }
    offs[tid + 1] = run;
    if (tid == 0) offs[0] = 0;
    __syncthreads();
    if (tid == 0) for (int t = 0; t < TPB; ++t) offs[t + 1] += offs[t];
    __syncthreads();
    double* cdf = a.cdf + (size_t)m * nb;
    double* centre = a.centre + (size_t)m * nb;
    run = offs[tid];
    for (int k = k0; k < k1; ++k) {
        run += cnt[k];
        if (a.counts) a.counts[(size_t)m * nb + k] = cnt[k];
        const double c = (double)run / (double)n_pix;
        cdf[k] = c;
        centre[k] = (edge(k) + edge(k + 1)) / 2.0;
        if (a.tcdf) a.newv[(size_t)m * nb + k] = interp_law(c, a.tcdf + (size_t)m * a.t_stride, a.tcentre + (size_t)m * a.t_stride, a.nt);
    }
}

// out = (float)interp((double)v, centre, new); sl[j] the slope of interval j
__device__ __forceinline__ float remap_one(float v, const double* __restrict__ sc, const double* __restrict__ sn, const double* __restrict__ sl,
                                           int nb, double inv) {
    const double x = (double)v;
    if (x < sc[0]) return (float)sn[0];
    if (x >= sc[nb - 1]) return (float)sn[nb - 1];
    const double g = (x - sc[0]) * inv;
    int j = g >= 0.0 ? (g < (double)(nb - 2) ? (int)g : nb - 2) : 0;       // a guess in [0, nb - 2], never trusted
    while (j > 0 && sc[j] > x) --j;
    while (j < nb - 2 && sc[j + 1] <= x) ++j;
    if (x == sc[j]) return (float)sn[j];
    return (float)(sl[j] * (x - sc[j]) + sn[j]);
}

// grid (nblk, n): block j of map m remaps pixels [j * chunk, (j + 1) * chunk) of maps into out (the same pixels; out may be maps)
__global__ __launch_bounds__(TPB) void hist_remap_kernel(HistArgs a) {
    __shared__ double sc[NBMAX], sn[NBMAX], sl[NBMAX];
    const int m = blockIdx.y, tid = threadIdx.x, nb = a.nb;
    const int n_pix = a.H * a.W;
    const double* centre = a.centre + (size_t)m * nb;
    const double* newv = a.newv + (size_t)m * nb;
    for (int k = tid; k < nb; k += TPB) {
        sc[k] = centre[k];
        sn[k] = newv[k];
        sl[k] = k + 1 < nb ? (newv[k + 1] - newv[k]) / (centre[k + 1] - centre[k]) : 0.0;
    }
    __syncthreads();
    const double inv = (double)(nb - 1) / (sc[nb - 1] - sc[0]);
    const int chunk = (n_pix + a.nblk - 1) / a.nblk;
    const int i0 = (int)min((long long)blockIdx.x * chunk, (long long)n_pix), i1 = (int)min((long long)i0 + chunk, (long long)n_pix);
    const int len = i1 - i0;
    if (len <= 0) return;
    const float* src = a.maps + (size_t)m * n_pix + i0;
    float* dst = a.out + (size_t)m * n_pix + i0;
    const uintptr_t as = (uintptr_t)src, ad = (uintptr_t)dst;
    const bool vec = ((as ^ ad) & 15) == 0;                // aligned alike: a head of 0 .. 3 floats, whole words, a tail
    const int head = vec ? min(len, (int)(((16 - (as & 15)) & 15) >> 2)) : len;
    const int words = (len - head) >> 2, tail0 = head + words * 4;
    for (int i = tid; i < head; i += TPB) dst[i] = remap_one(src[i], sc, sn, sl, nb, inv);
    const float4* s4 = reinterpret_cast<const float4*>(src + head);
    float4* d4 = reinterpret_cast<float4*>(dst + head);
    for (int q = tid; q < words; q += TPB) {
        const float4 v = s4[q];
        float4 o;
        o.x = remap_one(v.x, sc, sn, sl, nb, inv);
        o.y = remap_one(v.y, sc, sn, sl, nb, inv);
        o.z = remap_one(v.z, sc, sn, sl, nb, inv);
        o.w = remap_one(v.w, sc, sn, sl, nb, inv);
        d4[q] = o;
    }
    for (int i = tail0 + tid; i < len; i += TPB) dst[i] = remap_one(src[i], sc, sn, sl, nb, inv);
}

bool args_ok(const HistArgs& a) {
    if (a.n < 1 || a.n > 65535 || a.H < 1 || a.W < 1 || (long long)a.H * a.W > INT32_MAX || !a.maps) return false;
    if (a.kind != HIST_F32 && a.kind != HIST_DENSITY) return false;
    if (a.nb < 2 || a.nb > NBMAX) return false;
    if (!a.part || !a.mnmx || !a.counter || a.nblk != p3d_post_blocks((long long)a.H * a.W)) return false;
    if (!a.cnt || !a.cdf || !a.centre) return false;
    if (a.tcdf && (!a.tcentre || !a.newv || a.nt < 2 || a.nt > NBMAX || a.t_stride < 0)) return false;
    if (a.out && (!a.tcdf || a.kind != HIST_F32)) return false;
    return true;
}

}  // namespace

bool p3d_hist_has(int stage, const HistArgs& a) {
    switch (stage) {
        case HIST_MINMAX: case HIST_COUNT: return true;
        case HIST_REMAP: return a.out != nullptr;
        default: return false;
    }
}

LaunchDesc p3d_hist_desc(int stage, const HistArgs& a) {
    const double e = (double)a.n * a.H * a.W;
    switch (stage) {
        case HIST_MINMAX: return {"minmax_kernel", e * 2.0, e * 4.0};
        case HIST_COUNT: return {a.kind == HIST_DENSITY ? "hist_count_kernel<1>" : "hist_count_kernel<0>", e * 6.0, e * 4.0};      // one read
        default: return {"hist_remap_kernel", e * 6.0, e * 8.0};                                                                    // one read, one write
    }
}

hipError_t p3d_hist_launch(int stage, const HistArgs& a, hipStream_t s) {
    if (!args_ok(a) || stage < 0 || stage >= HIST_STAGES) return hipErrorInvalidValue;
    if (!p3d_hist_has(stage, a)) return hipSuccess;
    switch (stage) {
        case HIST_MINMAX: {
            PostArgs q;                                    // minmax_kernel, with this stage's own partials and result
            q.n = a.n; q.H = a.H; q.W = a.W; q.maps = const_cast<float*>(a.maps); q.norm = P3D_NORM_RANGE;
            q.part = a.part; q.mnmx = a.mnmx; q.counter = a.counter; q.nblk = a.nblk;
            return p3d_post_launch(POST_MINMAX, q, s);
        }
        case HIST_COUNT: {
            const hipError_t e = hipMemsetAsync(a.cnt, 0, (size_t)a.n * a.nb * sizeof(int), s);      // the tables start at zero, in stream order
            if (e != hipSuccess) return e;
            if (a.kind == HIST_DENSITY) hipLaunchKernelGGL(hist_count_kernel<HIST_DENSITY>, dim3(a.nblk, a.n), dim3(TPB), 0, s, a);
            else hipLaunchKernelGGL(hist_count_kernel<HIST_F32>, dim3(a.nblk, a.n), dim3(TPB), 0, s, a);
            break;
        }
        default:
            hipLaunchKernelGGL(hist_remap_kernel, dim3(a.nblk, a.n), dim3(TPB), 0, s, a);
    }
    return hipGetLastError();
}

hipError_t p3d_hist_chain_launch(const HistChain& c, hipStream_t s) {
    if (c.has_target)
        for (int st = HIST_MINMAX; st <= HIST_COUNT; ++st) {
            const hipError_t e = p3d_hist_launch(st, c.target, s);
            if (e != hipSuccess) return e;
        }
    for (int st = 0; st < HIST_STAGES; ++st) {
        const hipError_t e = p3d_hist_launch(st, c.source, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
