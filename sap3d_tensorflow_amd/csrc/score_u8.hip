// Scoring of 8-bit saliency maps against 8-bit ground truth (p3d_video_score, p3d_score_maps_u8; ScoreArgs in p3d_kernels.h, the
// law in include/p3d_hip.h, "Scoring 8-bit maps"): per map saliency s, density d and fixation x, [n_pix] bytes each.  On bytes
// CC, NSS and AUC-Judd follow from three 256-bin integer histograms and one integer sum of products, so no sort runs and no sum
// has an order; SIM and KL are sums over pixels of table entries.
//
//  * score_count_kernel (pass A): grid (nblk, n), block j of map m takes pixels [j * chunk, (j + 1) * chunk), chunk a multiple of
//    16.  Where the three sources of the block are aligned alike (ScoreCut) it reads whole 16-byte words between a head and a tail
//    of single pixels; otherwise every pixel is a byte load.  Saliency and density maps are extremely skewed, so, as in
//    hist_count_kernel, every wave owns a private LDS copy of the three tables and up to two candidate bins of a wave are counted
//    with one ballot each (a candidate held by four lanes or more retires with ONE add of their number); the fixated pixels are
//    few and add 1 each.  The products s * d are added per lane in 32 bits: a lane adds at most
//    2 + 16 * ceil(chunk / 16 / 256) <= 130 products of at most 255 * 255 (chunk <= 2^23 / 256 = 32768 rounded up to 16; the plan
//    hook reports the exact figure), far below the 66 051 that fit -- the trips are bounded, nothing is added in 64 bits before the
//    wave's fold.  Without a density map (no column that needs one: the sweeps of score_auc_u8.hip alone) the kernel's other
//    instantiation counts neither hd nor the products and reads two sources.  The copies are folded and flushed with integer atomics to the map's table (zeroed by the launcher in stream
//    order), the waves' 64-bit product sums likewise.
//    The last arriving block of a map (det_reduce.h's ticket) runs FINALISE on the tables alone, thread t on level v = 255 - t:
//    the moments are integer block sums, the two running sums of AUC-Judd are integer scans, CC / NSS / the REFERENCE-ties AUC are
//    one or two divisions of exactly known integers, the EXPECTED-ties AUC is a sum of 256 doubles in a fixed order (xor butterfly
//    over each wave, then ((w0 + w1) + w2) + w3), and the four 256-entry tables of pass B are built when SIM or KL is asked for.
//    AUC-Judd with every pixel fixated (n_f = n_pix) divides by zero in the reference; here it is NaN, and unpinned.
//  * score_terms_kernel (pass B): the map's four tables staged in LDS, one pixel per lane and pass; block partials through
//    write-through stores, folded in block order by the last arriver.
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
constexpr int TAB = 768;                                   // hs, hf, hd
static_assert(P3D_SCORE_TAB_WORDS == TAB + 2, "a map's tables are followed by its 64-bit sum of products");
constexpr double KL_EPS = 2.2204e-16;                      // utils/metrics.py:359, the literal

// one wave counts bin b of every lane (b < 0: the lane has none) into its own copy of one table
__device__ __forceinline__ void count_bin(unsigned* cnt, int b, int lane) {
    unsigned long long cand = __ballot(b >= 0);
    for (int round = 0; round < 2 && cand; ++round) {
        const int lead = __shfl(b, __ffsll((long long)cand) - 1);
        const unsigned long long same = __ballot(b == lead);
        if (__popcll(same) >= 4) {
            if (lane == __ffsll((long long)same) - 1) atomicAdd(&cnt[lead], (unsigned)__popcll(same));
            if (b == lead) b = -1;
        }
        cand &= ~same;
    }
    if (b >= 0) atomicAdd(&cnt[b], 1u);
}

// one pixel per lane (on: this lane holds one); -> its product.  DEN false: no density map, hd and the products are not counted
template <bool DEN>
__device__ __forceinline__ unsigned count_pixel(unsigned* cnt, bool on, unsigned s, unsigned d, unsigned x, int lane) {
    count_bin(cnt, on ? (int)s : -1, lane);
    if (DEN) count_bin(cnt + 512, on ? (int)d : -1, lane);
    if (on && x >= 128u) atomicAdd(&cnt[256 + s], 1u);
    return DEN && on ? s * d : 0u;
}

// pixels [lo, hi) of the block by byte loads, a wave-uniform trip count (the ballots need every lane)
template <bool DEN>
__device__ __forceinline__ unsigned count_range(unsigned* cnt, const unsigned char* ps, const unsigned char* pd, const unsigned char* px,
                                                int lo, int hi, int tid) {
    unsigned acc = 0u;
    for (int at = lo; at < hi; at += TPB) {
        const int i = at + tid;
        const bool on = i < hi;
        const unsigned s = on ? ps[i] : 0u, d = DEN && on ? pd[i] : 0u, x = on && px ? px[i] : 0u;
        acc += count_pixel<DEN>(cnt, on, s, d, x, tid & 63);
    }
    return acc;
}

__device__ __forceinline__ unsigned byte_of(const uint4& v, int j) {
    const unsigned w = (j >> 2) == 0 ? v.x : (j >> 2) == 1 ? v.y : (j >> 2) == 2 ? v.z : v.w;
    return (w >> ((j & 3) * 8)) & 255u;
}

__device__ __forceinline__ unsigned table_load(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// FINALISE of one map by its last arriving block; th: LDS room for the three tables
__device__ void score_finalise(const ScoreArgs& a, int m, unsigned* th, double* uu) {
    __shared__ long long wsum[WAVES][7];
    __shared__ unsigned wscan[WAVES][2];
    __shared__ unsigned long long occ[WAVES][2];
    __shared__ double wsd[WAVES], usum[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, v = 255 - tid;
    // the tables were bumped by device-scope atomics of other blocks: every read of them here is a device-scope load
    const unsigned* table = a.tab + (size_t)m * P3D_SCORE_TAB_WORDS;
    const unsigned hs = table_load(table + v), hf = table_load(table + 256 + v), hd = table_load(table + 512 + v);
    const long long sd = (long long)__hip_atomic_load(reinterpret_cast<const unsigned long long*>(table + TAB), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    th[v] = hs; th[256 + v] = hf; th[512 + v] = hd;
    // the moments (exact integers), and the inclusive sums over the levels >= v of hs and hf
    long long mo[6] = {(long long)v * hs, (long long)v * v * hs, (long long)v * hd, (long long)v * v * hd, (long long)hf, (long long)v * hf};
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int k = 0; k < 6; ++k) mo[k] += __shfl_xor(mo[k], o);
    unsigned A = hs, G = hf;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned ta = __shfl_up(A, o), tg = __shfl_up(G, o);
        if (lane >= o) { A += ta; G += tg; }
    }
    const unsigned long long os = __ballot(hs != 0u), od = __ballot(hd != 0u);
    if (lane == 63) {
#pragma unroll
        for (int k = 0; k < 6; ++k) wsum[wave][k] = mo[k];
        wscan[wave][0] = A; wscan[wave][1] = G;
        occ[wave][0] = os; occ[wave][1] = od;
    }
    __syncthreads();
    long long S1 = 0, S2 = 0, D1 = 0, D2 = 0, nf = 0, F1 = 0;
    for (int w = 0; w < WAVES; ++w) {
        S1 += wsum[w][0]; S2 += wsum[w][1]; D1 += wsum[w][2]; D2 += wsum[w][3]; nf += wsum[w][4]; F1 += wsum[w][5];
        if (w < wave) { A += wscan[w][0]; G += wscan[w][1]; }
    }
    const long long N = a.n_pix;
    const long long Gv = (long long)G - hf;                // fixated pixels above level v
    // AUC-Judd.  REFERENCE: the trapezoid sum over the swept points times 2 (N - nf) nf is the integer sum_v hs[v] w_v - nf^2,
    // w_v = 2 G_v + 1 while a fixation sits at or below v, else 2 nf.  EXPECTED: m[v] e(G_v, hf[v]).
    const long long iterm = (long long)hs * (Gv < nf ? 2 * Gv + 1 : 2 * nf);
    double eterm = 0.0;
    const long long mv = (long long)hs - hf;
    if (mv > 0 && nf > 0 && nf < N) {
        const double g = (double)Gv, f = (double)hf, dn = (double)nf;
        const double e = Gv + hf < nf ? (g + 0.5 + f / 2.0) / dn
                                      : (f * (g + 0.5) / dn + f * (f - 1.0) / (2.0 * dn) + 1.0) / (f + 1.0);
        eterm = (double)mv * e;
    }
    long long isum = iterm;
    for (int o = 32; o > 0; o >>= 1) isum += __shfl_xor(isum, o);
    if (lane == 0) wsum[wave][6] = isum;
    const double esum = p3d_block_sum<false>(eterm, wsd);  // (its barrier publishes wsum[.][6] too)
    isum = ((wsum[0][6] + wsum[1][6]) + wsum[2][6]) + wsum[3][6];
    double* out = a.out + (size_t)m * 5;
    if (tid == 0) {
        const long long vs = N * S2 - S1 * S1, vd = N * D2 - D1 * D1;
        double cc = NAN, nss = NAN, auc = NAN;
        if (vs != 0 && vd != 0) cc = (double)(N * sd - S1 * D1) / (sqrt((double)vs) * sqrt((double)vd));
        if (nf != 0 && vs != 0) nss = (double)(N * F1 - nf * S1) / ((double)nf * sqrt((double)vs));
        if (nf != 0 && nf != N)
            auc = a.ties == P3D_SCORE_TIES_REFERENCE ? (double)(isum - nf * nf) / (double)(2 * (N - nf) * nf) : esum / (double)(N - nf);
        out[0] = (a.flags & P3D_SCORE_CC) ? cc : NAN;
        out[1] = NAN;
        out[2] = (a.flags & P3D_SCORE_JUDD) ? auc : NAN;
        out[3] = NAN;
        out[4] = (a.flags & P3D_SCORE_NSS) ? nss : NAN;
    }
    if (!(a.flags & (P3D_SCORE_SIM | P3D_SCORE_KL))) return;
    // the tables of pass B.  Lowest / highest occupied levels: thread t holds level 255 - t, so bit l of wave w is level 255 - 64 w - l
    int mn[2] = {0, 0}, mx[2] = {0, 0};
    for (int k = 0; k < 2; ++k) {
        bool seen = false;
        for (int w = 0; w < WAVES; ++w) {
            const unsigned long long b = occ[w][k];
            if (!b) continue;
            if (!seen) { mx[k] = 255 - 64 * w - (__ffsll((long long)b) - 1); seen = true; }
            mn[k] = 255 - 64 * w - (63 - __clzll((long long)b));
        }
    }
    uu[v] = (double)(v - mn[0]) / (double)(mx[0] - mn[0]);
    uu[256 + v] = (double)(v - mn[1]) / (double)(mx[1] - mn[1]);
    __syncthreads();
    if (lane == 0 && wave < 2) {                           // U of the saliency (wave 0) and of the density (wave 1): ascending levels
        double U = 0.0;
        for (int u = 0; u < 256; ++u) {
            const unsigned c = th[wave * 512 + u];
            if (c) U = U + (double)c * uu[wave * 256 + u];
        }
        usum[wave] = U;
    }
    __syncthreads();
    double* lut = a.lut + (size_t)m * 1024;
    lut[v] = uu[v] / usum[0];
    lut[256 + v] = uu[256 + v] / usum[1];
    lut[512 + v] = S1 ? (double)v / (double)S1 : 0.0;
    lut[768 + v] = D1 ? (double)v / (double)D1 : 0.0;
}

template <bool DEN>
__global__ __launch_bounds__(TPB) void score_count_kernel(ScoreArgs a) {
    __shared__ unsigned cnt[WAVES * TAB];
    __shared__ double uu[512];
    __shared__ int last;
    const int m = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    for (int k = tid; k < WAVES * TAB; k += TPB) cnt[k] = 0u;
    __syncthreads();
    const int i0 = (int)min((long long)blockIdx.x * a.chunk, (long long)a.n_pix), i1 = (int)min((long long)i0 + a.chunk, (long long)a.n_pix);
    const int len = i1 - i0;
    const unsigned char* ps = a.sal + (size_t)m * a.n_pix + i0;
    const unsigned char* pd = DEN ? a.den + (size_t)m * a.n_pix + i0 : ps;
    const unsigned char* px = a.fix ? a.fix + (size_t)m * a.n_pix + i0 : nullptr;
    unsigned* mine = cnt + (tid >> 6) * TAB;
    const ScoreCut cut = p3d_score_cut((uintptr_t)ps, (uintptr_t)pd, px ? (uintptr_t)px : (uintptr_t)ps, len);      // block-uniform
    unsigned acc = count_range<DEN>(mine, ps, pd, px, 0, cut.head, tid);
    const uint4* s4 = reinterpret_cast<const uint4*>(ps + cut.head);
    const uint4* d4 = reinterpret_cast<const uint4*>(pd + cut.head);
    const uint4* x4 = reinterpret_cast<const uint4*>(px ? px + cut.head : ps + cut.head);
    for (int at = 0; at < cut.words; at += TPB) {
        const int q = at + tid;
        const bool on = q < cut.words;
        uint4 vs = {0u, 0u, 0u, 0u}, vd = vs, vx = vs;
        if (on) { vs = s4[q]; if (DEN) vd = d4[q]; if (px) vx = x4[q]; }
#pragma unroll
        for (int j = 0; j < 16; ++j) acc += count_pixel<DEN>(mine, on, byte_of(vs, j), byte_of(vd, j), byte_of(vx, j), lane);
    }
    acc += count_range<DEN>(mine, ps, pd, px, cut.head + cut.words * 16, len, tid);
    __syncthreads();
    unsigned* table = a.tab + (size_t)m * P3D_SCORE_TAB_WORDS;
    for (int k = tid; k < TAB; k += TPB) {
        unsigned tot = 0u;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) tot += cnt[w * TAB + k];
        if (tot) __hip_atomic_fetch_add(&table[k], tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    unsigned long long tot = acc;
    for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o);
    if (lane == 0 && tot) __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(table + TAB), tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!p3d_last_block_wt(a.counter + m, a.nblk, &last)) return;
    score_finalise(a, m, cnt, uu);
}

// min(a, b) that keeps a NaN of either side, as np.minimum does
__device__ __forceinline__ double min_nan(double x, double y) { return x < y ? x : (y <= x ? y : x + y); }

__global__ __launch_bounds__(TPB) void score_terms_kernel(ScoreArgs a) {
    __shared__ double lut[1024];
    __shared__ double wsum[WAVES];
    __shared__ int last;
    const int m = blockIdx.y, tid = threadIdx.x;
    const double* src = a.lut + (size_t)m * 1024;
    for (int k = tid; k < 1024; k += TPB) lut[k] = src[k];
    __syncthreads();
    const int i0 = (int)min((long long)blockIdx.x * a.chunk, (long long)a.n_pix), i1 = (int)min((long long)i0 + a.chunk, (long long)a.n_pix);
    const unsigned char* ps = a.sal + (size_t)m * a.n_pix;
    const unsigned char* pd = a.den + (size_t)m * a.n_pix;
    const bool want_sim = a.flags & P3D_SCORE_SIM, want_kl = a.flags & P3D_SCORE_KL;
    double sim = 0.0, kl = 0.0;
    for (int i = i0 + tid; i < i1; i += TPB) {
        const unsigned s = ps[i], d = pd[i];
        if (want_sim) sim = sim + min_nan(lut[s], lut[256 + d]);
        if (want_kl) {
            const double q = lut[768 + d];
            kl = kl + q * log(KL_EPS + q / (lut[512 + s] + KL_EPS));
        }
    }
    const double bs = p3d_block_sum<false>(sim, wsum);
    const double bk = p3d_block_sum<true>(kl, wsum);
    double* part = a.part + (size_t)m * a.nblk * 2;
    if (tid == 0) { p3d_store_wt(part, (size_t)blockIdx.x * 2, bs); p3d_store_wt(part, (size_t)blockIdx.x * 2 + 1, bk); }
    if (!p3d_last_block_wt(a.counter + a.n + m, a.nblk, &last)) return;
    if (tid == 0) {
        double S = 0.0, K = 0.0;
        for (int j = 0; j < a.nblk; ++j) { S = S + part[j * 2]; K = K + part[j * 2 + 1]; }
        if (want_sim) a.out[(size_t)m * 5 + 1] = S;
        if (want_kl) a.out[(size_t)m * 5 + 3] = K;
    }
}

bool args_ok(const ScoreArgs& a) {
    if (a.n < 1 || a.n > 65535 || a.n_pix < 1 || a.n_pix > P3D_SCORE_MAX_PIXELS || !a.sal) return false;
    if (a.flags < 0 || (a.flags & ~P3D_SCORE_ALL)) return false;
    if (!a.den && (a.flags & (P3D_SCORE_CC | P3D_SCORE_SIM | P3D_SCORE_KL))) return false;
    if (a.ties != P3D_SCORE_TIES_REFERENCE && a.ties != P3D_SCORE_TIES_EXPECTED) return false;
    if (!a.fix && (a.flags & (P3D_SCORE_JUDD | P3D_SCORE_NSS))) return false;
    const ScorePlan p = p3d_score_plan(a.n_pix);
    if (a.nblk != p.nblk || a.chunk != p.chunk) return false;
    if (!a.tab || !a.counter || !a.out) return false;
    if ((a.flags & (P3D_SCORE_SIM | P3D_SCORE_KL)) && (!a.lut || !a.part)) return false;
    return true;
}

}  // namespace

ScorePlan p3d_score_plan(long long n_pix) {
    ScorePlan p;
    const long long blocks = std::max<long long>(1, std::min<long long>((n_pix + 32767) / 32768, 256));
    p.chunk = (int)((((n_pix + blocks - 1) / blocks) + 15) / 16 * 16);
    p.nblk = (int)((n_pix + p.chunk - 1) / p.chunk);       // no block is empty
    return p;
}

long long p3d_score_lane_products(long long n_pix, int n, unsigned off_s, unsigned off_d, unsigned off_x) {
    const ScorePlan p = p3d_score_plan(n_pix);
    long long worst = 0;
    for (int m = 0; m < n; ++m)
        for (int j = 0; j < p.nblk; ++j) {
            const long long i0 = (long long)j * p.chunk, at = (long long)m * n_pix + i0;
            const int len = (int)std::min<long long>(p.chunk, n_pix - i0);
            const ScoreCut c = p3d_score_cut((uintptr_t)(off_s + at), (uintptr_t)(off_d + at), (uintptr_t)(off_x + at), len);
            const int tail = len - c.head - c.words * 16;
            worst = std::max<long long>(worst, (c.head + TPB - 1) / TPB + (long long)((c.words + TPB - 1) / TPB) * 16 + (tail + TPB - 1) / TPB);
        }
    return worst;
}

bool p3d_score_has(int stage, const ScoreArgs& a) {
    switch (stage) {
        case SCORE_COUNT: return true;
        case SCORE_TERMS: return (a.flags & (P3D_SCORE_SIM | P3D_SCORE_KL)) != 0;
        default: return false;
    }
}

LaunchDesc p3d_score_desc(int stage, const ScoreArgs& a) {
    const double e = (double)a.n * (double)a.n_pix;
    if (stage == SCORE_COUNT) return {"score_count_kernel", e * 2.0, e * ((a.fix ? 2.0 : 1.0) + (a.den ? 1.0 : 0.0))};      // one read of every source
    return {"score_terms_kernel", e * 8.0, e * 2.0};
}

hipError_t p3d_score_launch(int stage, const ScoreArgs& a, hipStream_t s) {
    if (!args_ok(a) || stage < 0 || stage >= SCORE_STAGES) return hipErrorInvalidValue;
    if (!p3d_score_has(stage, a)) return hipSuccess;
    if (stage == SCORE_COUNT) {
        const hipError_t e = hipMemsetAsync(a.tab, 0, (size_t)a.n * P3D_SCORE_TAB_WORDS * sizeof(unsigned), s);      // the tables start at zero, in stream order
        if (e != hipSuccess) return e;
        if (a.den) hipLaunchKernelGGL(score_count_kernel<true>, dim3(a.nblk, a.n), dim3(TPB), 0, s, a);
        else hipLaunchKernelGGL(score_count_kernel<false>, dim3(a.nblk, a.n), dim3(TPB), 0, s, a);
    } else {
        hipLaunchKernelGGL(score_terms_kernel, dim3(a.nblk, a.n), dim3(TPB), 0, s, a);
    }
    return hipGetLastError();
}
