// AUC-Borji and shuffled AUC of 8-bit saliency maps (p3d_score_sweep_u8, p3d_video_score_auc; ScoreSweepArgs in p3d_kernels.h, the
// law in include/p3d_hip.h, "SPLIT SWEEP").  On bytes the curve of a split depends only on integer counts per threshold level: the
// fixation side comes from hf of score_u8.hip's pass A, the random side is a gather of n_rows bytes per split.  No pass over the
// map runs here and nothing is added in floating point before the one lane that walks a split's points.
//
//  * sweep_prep_kernel (SWEEP_PREP): one block per map, thread v on level v of pass A's tables.  lo / hi / maxfix from ballots, u_v,
//    lev[v] by a binary search over k (t_k = k * step does not decrease with k, so the count of t_k <= u_v is the first k with
//    t_k > u_v), the suffix sums of hf by a scan in LDS, and the ladder lad[l] = sum of hf[v] over lev[v] >= l, l = 0 .. kmax: lev
//    does not decrease with v, so it is the suffix sum at the first v with lev[v] >= l.  info[m] = {nf, lo, hi, maxfix}.
//  * sweep_run_kernel (SWEEP_RUN): grid (ceil(n_rep / S), n).  idx is [n_rows][n_rep] row-major -- consecutive ints are consecutive
//    splits of one row -- so lanes run along SPLITS: thread (r, j) of a block of S split columns and 256 / S row lanes reads
//    idx[row][s0 + j] for rows r, r + 256 / S, ..., S consecutive ints per row (coalesced), gathers the byte and adds 1 to its
//    level in split j's own histogram in LDS (integer atomics; kmax + 1 counters per split, S sized so that they fit), and keeps
//    the largest byte.  After one barrier lane j of the first wave walks split j's K points in the law's order.
#include "p3d_kernels.h"
#include "../../include/p3d_hip.h"
#include <math.h>
#include <algorithm>

// every product, quotient and sum below rounds on its own (the header's law): hipcc would otherwise fuse a * b + c
#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr int SWEEP_LDS_BYTES = 48 * 1024;               // the splits' histograms of one block
constexpr int SWEEP_MAX_COLS = 32;                       // split columns per block: 128-byte row segments, 8 row lanes

__device__ __forceinline__ unsigned table_load(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(TPB) void sweep_prep_kernel(ScoreSweepArgs a) {
    __shared__ unsigned long long occ[WAVES][2];
    __shared__ unsigned sfx[2][256];
    __shared__ int slev[256];
    const int m = blockIdx.x, v = threadIdx.x, lane = v & 63, wave = v >> 6;
    // the tables were bumped by device-scope atomics of another launch's blocks
    const unsigned* table = a.tab + (size_t)m * P3D_SCORE_TAB_WORDS;
    const unsigned hs = table_load(table + v), hf = table_load(table + 256 + v);
    const unsigned long long os = __ballot(hs != 0u), of = __ballot(hf != 0u);
    if (lane == 0) { occ[wave][0] = os; occ[wave][1] = of; }
    sfx[0][v] = hf;
    __syncthreads();
    int lo = -1, hi = -1, maxfix = -1;                      // bit l of wave w is level 64 w + l
    for (int w = 0; w < WAVES; ++w) {
        const unsigned long long b = occ[w][0], f = occ[w][1];
        if (b) { if (lo < 0) lo = 64 * w + __ffsll((long long)b) - 1; hi = 64 * w + 63 - __clzll((long long)b); }
        if (f) maxfix = 64 * w + 63 - __clzll((long long)f);
    }
    // inclusive suffix sums of hf: sfx[.][v] = sum over u >= v
    int cur = 0;
    for (int o = 1; o < 256; o <<= 1) {
        const unsigned x = sfx[cur][v] + (v + o < 256 ? sfx[cur][v + o] : 0u);
        sfx[cur ^ 1][v] = x;
        cur ^= 1;
        __syncthreads();
    }
    int lev = 0;
    if (hi > lo) {
        const double u = (double)(v - lo) / (double)(hi - lo);
        int l0 = 0, l1 = a.kmax;                            // the first k in [0, kmax] with t_k > u (kmax: none)
        while (l0 < l1) {
            const int mid = (l0 + l1) >> 1;
            if ((double)mid * a.step <= u) l0 = mid + 1; else l1 = mid;
        }
        lev = l0;
    }
    slev[v] = lev;
    a.lev[(size_t)m * 256 + v] = lev;
    if (v == 0) {
        int* info = a.info + (size_t)m * 4;
        info[0] = (int)sfx[cur][0]; info[1] = lo; info[2] = hi; info[3] = maxfix;
    }
    __syncthreads();
    unsigned* lad = a.lad + (size_t)m * (a.kmax + 1);
    for (int l = v; l <= a.kmax; l += TPB) {
        int v0 = 0, v1 = 256;                               // the first level in [0, 256] with lev >= l (256: none)
        while (v0 < v1) {
            const int mid = (v0 + v1) >> 1;
            if (slev[mid] >= l) v1 = mid; else v0 = mid + 1;
        }
        lad[l] = v0 < 256 ? sfx[cur][v0] : 0u;
    }
}

__global__ __launch_bounds__(TPB) void sweep_run_kernel(ScoreSweepArgs a) {
    extern __shared__ unsigned hist[];                      // [cols][kmax + 1]
    __shared__ int slev[256];
    __shared__ int stop[SWEEP_MAX_COLS];
    const int m = blockIdx.y, tid = threadIdx.x, cols = a.cols, nl = a.kmax + 1;
    const int j = tid & (cols - 1), r = tid / cols, rlanes = TPB / cols;
    const int split = blockIdx.x * cols + j;
    for (int k = tid; k < cols * nl; k += TPB) hist[k] = 0u;
    slev[tid] = a.lev[(size_t)m * 256 + tid];
    if (tid < SWEEP_MAX_COLS) stop[tid] = -1;
    __syncthreads();
    const int n_rows = (int)a.meta[(size_t)m * 2];
    const int* idx = a.idx + a.meta[(size_t)m * 2 + 1];
    const unsigned char* ps = a.sal + (size_t)m * a.n_pix;
    if (split < a.n_rep) {
        unsigned* cnt = hist + j * nl;                      // split j's own counters
        int top = -1;
        for (int row = r; row < n_rows; row += rlanes) {
            const int b = ps[idx[(size_t)row * a.n_rep + split]];
            atomicAdd(&cnt[slev[b]], 1u);
            top = max(top, b);
        }
        if (top >= 0) atomicMax(&stop[j], top);
    }
    __syncthreads();
    if (r != 0 || split >= a.n_rep) return;
    const int* info = a.info + (size_t)m * 4;
    const int nf = info[0], lo = info[1], hi = info[2];
    const int top = max(info[3], stop[j]);
    if (a.top) a.top[(size_t)m * a.n_rep + split] = top;
    double* out = a.per_rep + (size_t)m * a.n_rep + split;
    if (nf == 0 || hi == lo) { *out = NAN; return; }
    const double dn = (double)nf;
    const double u_top = (double)(top - lo) / (double)(hi - lo);
    const int K = u_top == 0.0 ? 0 : (int)ceil(u_top / a.step);
    const unsigned* lad = a.lad + (size_t)m * nl;
    const unsigned* mine = hist + j * nl;
    unsigned cfp = 0u;
    double px = 0.0, py = 0.0, area = 0.0;
    for (int l = a.kmax; l >= 1; --l) {                     // the counts of level l join before point k = l - 1 is taken
        cfp += mine[l];
        if (l - 1 >= K) continue;
        const double x = (double)cfp / dn, y = (double)lad[l] / dn;
        area = area + (x - px) * (y + py) * 0.5;
        px = x; py = y;
    }
    area = area + (1.0 - px) * (1.0 + py) * 0.5;
    *out = area;
}

bool args_ok(int stage, const ScoreSweepArgs& a) {
    if (a.n < 1 || a.n > 65535 || a.n_pix < 1 || a.n_pix > P3D_SCORE_MAX_PIXELS) return false;
    if (!(a.step > 0.0) || a.kmax != p3d_sweep_kmax(a.step) || a.kmax < 1 || a.kmax > P3D_SWEEP_MAX_KMAX) return false;
    if (!a.lev || !a.lad || !a.info) return false;
    if (stage == SWEEP_PREP) return a.tab != nullptr;
    if (a.n_rep < 1 || a.cols != p3d_sweep_cols(a.kmax, a.n_rep)) return false;
    return a.sal && a.idx && a.meta && a.per_rep;
}

}  // namespace

int p3d_sweep_kmax(double step) {
    if (!(step > 0.0)) return 0;
    const double k = ceil(1.0 / step);
    return k > (double)P3D_SWEEP_MAX_KMAX ? 0 : (int)k;
}

int p3d_sweep_cols(int kmax, int n_rep) {
    int cols = SWEEP_MAX_COLS;
    while (cols > 1 && ((size_t)cols * (kmax + 1) * sizeof(unsigned) > (size_t)SWEEP_LDS_BYTES || cols / 2 >= n_rep)) cols >>= 1;
    return cols;
}

LaunchDesc p3d_sweep_desc(int stage, const ScoreSweepArgs& a) {
    if (stage == SWEEP_PREP) return {"sweep_prep_kernel", (double)a.n * 256.0 * 12.0, (double)a.n * (2048.0 + 1024.0 + 4.0 * (a.kmax + 1))};
    return {"sweep_run_kernel", (double)a.n * a.n_rep * a.kmax * 8.0, (double)a.n * 1024.0};      // plus 5 bytes per gathered sample
}

hipError_t p3d_sweep_launch(int stage, const ScoreSweepArgs& a, hipStream_t s) {
    if (stage < 0 || stage >= SWEEP_STAGES || !args_ok(stage, a)) return hipErrorInvalidValue;
    if (stage == SWEEP_PREP) {
        hipLaunchKernelGGL(sweep_prep_kernel, dim3(a.n), dim3(TPB), 0, s, a);
    } else {
        const size_t lds = (size_t)a.cols * (a.kmax + 1) * sizeof(unsigned);
        hipLaunchKernelGGL(sweep_run_kernel, dim3((a.n_rep + a.cols - 1) / a.cols, a.n), dim3(TPB), lds, s, a);
    }
    return hipGetLastError();
}
