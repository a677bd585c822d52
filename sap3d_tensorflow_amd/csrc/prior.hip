// Fixation priors built on the device (p3d_prior_*, p3d_set_prior_stage; PriorCountArgs / PriorApplyArgs in p3d_kernels.h, the law
// in include/p3d_hip.h): 8-bit maps are counted into one uint32 accumulator per pixel, the counts become a float32 map that
// goes through postprocess.hip's blur and max-normalisation, and that map multiplies or mixes into output maps as POST_PRIOR.
//
//  * prior_count_kernel<KIND>: grid (lanes / 256, slices).  A word lane owns four consecutive pixels whose bytes form one aligned
//    32-bit word in every map (n_pix % 4 == 0: the alignment of pixel p is then the same in every map); it walks the maps of its
//    slice in ascending order, UNROLL loads in flight, sums in four registers and touches the accumulator once.  The 0 .. 3
//    pixels ahead of the first aligned word, those after the last whole word, and every pixel when n_pix % 4 != 0 belong to byte
//    lanes, one pixel each, the same walk on single bytes.  One slice: the lane is the only writer of its words, a plain
//    read-modify-write.  More (a pixel grid that alone would not fill the chip): the slices meet in integer atomic adds.
//    Counts are integers and wrap modulo 2^32, so neither the cut nor the arrival order can show.  A subtraction that finds less
//    than it takes away raises *flag by a plain store of 1 (whoever stores, the value is the same) and carries on: whatever the
//    order of the slices, some subtraction sees the shortfall exactly when the total exceeds what was there.
//  * prior_float_kernel: c_i = (float)count_i, round to nearest even (exact below 2^24).
//  * prior_apply_kernel<MODE>: grid (nblk, n), block j of map m owns pixels [j * chunk, (j + 1) * chunk) of the map and of the
//    prior; one lane per element, 16 bytes per lane where the two are aligned alike (a head of 0 .. 3 floats, whole words, a
//    tail), element by element otherwise.  In place; every element is read and written by exactly one lane.
#include "p3d_kernels.h"
#include "../../include/p3d_hip.h"
#include <algorithm>

// every product and sum below rounds on its own (the header's fmul / fadd): hipcc would otherwise fuse a * b + c
#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr int UNROLL = 8;                                  // maps in flight per lane
constexpr long long FILL_BLOCKS = 1024;                    // blocks the map-sliced launch aims at (256 CUs, four blocks each)
constexpr long long SLICE_MIN_MAPS = 8;                    // a slice is worth its atomics from this many maps on
static_assert(P3D_PRIOR_KIND_FIXATIONS == P3D_PRIOR_FIXATIONS && P3D_PRIOR_KIND_BYTES == P3D_PRIOR_BYTES, "the ABI names the kernels' kinds");
static_assert(P3D_PRIOR_STAGE_MUL == P3D_PRIOR_MUL && P3D_PRIOR_STAGE_MIX == P3D_PRIOR_MIX, "the ABI names the kernels' modes");

template <int KIND>
__device__ __forceinline__ unsigned tally(unsigned byte) { return KIND == P3D_PRIOR_KIND_FIXATIONS ? (byte >= 128u ? 1u : 0u) : byte; }

// pixel p of the accumulator takes +v or -v; one slice: this lane is the word's only writer
__device__ __forceinline__ void commit(const PriorCountArgs& a, long long p, unsigned v) {
    if (v == 0u) return;
    unsigned old;
    if (a.slices == 1) {
        old = a.count[p];
        a.count[p] = a.sign > 0 ? old + v : old - v;
    } else {
        const unsigned add = a.sign > 0 ? v : 0u - v;
        old = __hip_atomic_fetch_add(&a.count[p], add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (a.sign < 0 && old < v) *a.flag = 1u;
}

template <int KIND>
__global__ __launch_bounds__(TPB) void prior_count_kernel(PriorCountArgs a) {
    const long long lane = (long long)blockIdx.x * TPB + threadIdx.x;
    if (lane >= a.words + a.singles) return;
    const long long m0 = (long long)blockIdx.y * a.per_slice, m1 = min(a.n, m0 + a.per_slice);
    if (lane < a.words) {
        const long long p = a.head + 4 * lane;
        const unsigned char* src = a.maps + p;             // 4-byte aligned in every map (the launcher's head)
        unsigned c0 = 0u, c1 = 0u, c2 = 0u, c3 = 0u;
        long long m = m0;
        for (; m + UNROLL <= m1; m += UNROLL) {
            unsigned w[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) w[u] = *reinterpret_cast<const unsigned*>(src + (m + u) * a.n_pix);
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                c0 += tally<KIND>(w[u] & 255u); c1 += tally<KIND>((w[u] >> 8) & 255u);
                c2 += tally<KIND>((w[u] >> 16) & 255u); c3 += tally<KIND>(w[u] >> 24);
            }
        }
        for (; m < m1; ++m) {
            const unsigned w = *reinterpret_cast<const unsigned*>(src + m * a.n_pix);
            c0 += tally<KIND>(w & 255u); c1 += tally<KIND>((w >> 8) & 255u); c2 += tally<KIND>((w >> 16) & 255u); c3 += tally<KIND>(w >> 24);
        }
        commit(a, p, c0); commit(a, p + 1, c1); commit(a, p + 2, c2); commit(a, p + 3, c3);
    } else {
        const long long k = lane - a.words;                // the head's pixels first, then those behind the last whole word
        const long long p = k < a.head ? k : 4 * a.words + k;
        const unsigned char* src = a.maps + p;
        unsigned c = 0u;
        long long m = m0;
        for (; m + UNROLL <= m1; m += UNROLL) {
            unsigned b[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) b[u] = src[(m + u) * a.n_pix];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) c += tally<KIND>(b[u]);
        }
        for (; m < m1; ++m) c += tally<KIND>(src[m * a.n_pix]);
        commit(a, p, c);
    }
}

__global__ __launch_bounds__(TPB) void prior_float_kernel(const unsigned* __restrict__ count, float* __restrict__ out, long long n_pix) {
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n_pix; i += (long long)gridDim.x * TPB) out[i] = __uint2float_rn(count[i]);
}

template <int MODE>
__device__ __forceinline__ float prior_law(float v, float g, float a, float b) {
    return MODE == P3D_PRIOR_STAGE_MUL ? v * (b * g + a) : b * v + a * g;
}

template <int MODE>
__global__ __launch_bounds__(TPB) void prior_apply_kernel(PriorApplyArgs q) {
    const int m = blockIdx.y, tid = threadIdx.x;
    const int chunk = (q.n_pix + q.nblk - 1) / q.nblk;
    const int i0 = (int)min((long long)blockIdx.x * chunk, (long long)q.n_pix), i1 = (int)min((long long)i0 + chunk, (long long)q.n_pix);
    const int len = i1 - i0;
    if (len <= 0) return;
    float* v = q.maps + (size_t)m * q.n_pix + i0;
    const float* g = q.prior + i0;
    const uintptr_t av = (uintptr_t)v, ag = (uintptr_t)g;
    const bool vec = ((av ^ ag) & 15) == 0;                // aligned alike: a head of 0 .. 3 floats, whole words, a tail
    const int head = vec ? min(len, (int)(((16 - (av & 15)) & 15) >> 2)) : len;
    const int words = (len - head) >> 2, tail0 = head + words * 4;
    for (int i = tid; i < head; i += TPB) v[i] = prior_law<MODE>(v[i], g[i], q.a, q.b);
    float4* v4 = reinterpret_cast<float4*>(v + head);
    const float4* g4 = reinterpret_cast<const float4*>(g + head);
    for (int k = tid; k < words; k += TPB) {
        const float4 x = v4[k], y = g4[k];
        float4 o;
        o.x = prior_law<MODE>(x.x, y.x, q.a, q.b);
        o.y = prior_law<MODE>(x.y, y.y, q.a, q.b);
        o.z = prior_law<MODE>(x.z, y.z, q.a, q.b);
        o.w = prior_law<MODE>(x.w, y.w, q.a, q.b);
        v4[k] = o;
    }
    for (int i = tail0 + tid; i < len; i += TPB) v[i] = prior_law<MODE>(v[i], g[i], q.a, q.b);
}

}  // namespace

// The cut of one count launch: words / singles / head from the base's alignment, slices from the pixel grid and the map count.
// False: arguments the kernel must not see.
bool p3d_prior_count_plan(PriorCountArgs& a) {
    if (!a.maps || !a.count || !a.flag || a.n < 1 || a.n > P3D_PRIOR_MAPS_CAP || a.n_pix < 1 || a.n_pix > INT32_MAX) return false;
    if (a.kind != P3D_PRIOR_KIND_FIXATIONS && a.kind != P3D_PRIOR_KIND_BYTES) return false;
    if (a.sign != 1 && a.sign != -1) return false;
    if ((uintptr_t)a.count & 3 || (uintptr_t)a.flag & 3) return false;
    if (a.n_pix % 4 == 0) {
        a.head = std::min<long long>(a.n_pix, (long long)((4 - ((uintptr_t)a.maps & 3)) & 3));
        a.words = (a.n_pix - a.head) / 4;
    } else {
        a.head = 0; a.words = 0;                           // map m starts at m * n_pix: its alignment changes from map to map
    }
    a.singles = a.n_pix - 4 * a.words;
    const long long blocks = (a.words + a.singles + TPB - 1) / TPB;
    long long slices = 1;
    if (blocks < FILL_BLOCKS) slices = std::min((a.n + SLICE_MIN_MAPS - 1) / SLICE_MIN_MAPS, (FILL_BLOCKS + blocks - 1) / blocks);
    slices = std::max<long long>(1, std::min<long long>(slices, 65535));
    a.per_slice = (a.n + slices - 1) / slices;
    a.slices = (int)((a.n + a.per_slice - 1) / a.per_slice);       // no empty slice
    return blocks <= INT32_MAX;
}

LaunchDesc p3d_prior_count_desc(const PriorCountArgs& a) {
    const double e = (double)a.n * (double)a.n_pix;
    return {a.kind == P3D_PRIOR_KIND_BYTES ? "prior_count_kernel<1>" : "prior_count_kernel<0>", e, e + 8.0 * (double)a.n_pix * a.slices};
}

hipError_t p3d_prior_count_launch(const PriorCountArgs& args, hipStream_t s) {
    PriorCountArgs a = args;
    if (!p3d_prior_count_plan(a)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.words + a.singles + TPB - 1) / TPB), (unsigned)a.slices);
    if (a.kind == P3D_PRIOR_KIND_BYTES) hipLaunchKernelGGL(prior_count_kernel<P3D_PRIOR_KIND_BYTES>, grid, dim3(TPB), 0, s, a);
    else hipLaunchKernelGGL(prior_count_kernel<P3D_PRIOR_KIND_FIXATIONS>, grid, dim3(TPB), 0, s, a);
    return hipGetLastError();
}

hipError_t p3d_prior_float(const unsigned* count, float* out, long long n_pix, hipStream_t s) {
    if (!count || !out || n_pix < 1 || n_pix > INT32_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(prior_float_kernel, dim3((unsigned)std::min<long long>((n_pix + TPB - 1) / TPB, 65535)), dim3(TPB), 0, s, count, out, n_pix);
    return hipGetLastError();
}

LaunchDesc p3d_prior_apply_desc(const PriorApplyArgs& q) {
    const double e = (double)q.n * q.n_pix;
    return {q.mode == P3D_PRIOR_STAGE_MUL ? "prior_apply_kernel<1>" : "prior_apply_kernel<2>", e * 3.0, e * 12.0};
}

hipError_t p3d_prior_apply_launch(const PriorApplyArgs& q, hipStream_t s) {
    if (!q.maps || !q.prior || q.n < 1 || q.n > 65535 || q.n_pix < 1) return hipErrorInvalidValue;
    if (q.mode != P3D_PRIOR_STAGE_MUL && q.mode != P3D_PRIOR_STAGE_MIX) return hipErrorInvalidValue;
    if (q.nblk != p3d_post_blocks(q.n_pix) || !(q.a >= 0.f && q.a <= 1.f) || !(q.b >= 0.f && q.b <= 1.f)) return hipErrorInvalidValue;
    if ((uintptr_t)q.maps & 3 || (uintptr_t)q.prior & 3) return hipErrorInvalidValue;
    if (q.mode == P3D_PRIOR_STAGE_MUL) hipLaunchKernelGGL(prior_apply_kernel<P3D_PRIOR_STAGE_MUL>, dim3(q.nblk, q.n), dim3(TPB), 0, s, q);
    else hipLaunchKernelGGL(prior_apply_kernel<P3D_PRIOR_STAGE_MIX>, dim3(q.nblk, q.n), dim3(TPB), 0, s, q);
    return hipGetLastError();
}
