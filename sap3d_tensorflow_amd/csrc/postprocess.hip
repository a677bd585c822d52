// Smoothing and normalisation of output maps (p3d_set_postprocess; PostArgs in p3d_kernels.h, the contract in include/p3d_hip.h):
// a separable Gaussian of up to 511 taps on float32 maps at output resolution, then each map scaled by its maximum or to its
// range, then -- for images -- the byte law of resize_u8_kernel.
//
//  * blur_h_kernel: a block owns up to SEG consecutive outputs of one row and stages them with r halo elements on either side
//    in LDS; the reflection (reflect-101) is resolved while loading, the loads and the stores run along x.
//  * blur_v_kernel: a block owns cols columns x rows output rows and stages (rows + 2r) x cols in LDS, every staged row one
//    run of cols consecutive floats.  cols shrinks as r grows so that the strip fits 64 KB (p3d_post_strip, host only).
//  In both, the r + 1 weights w[r .. 2r] sit in LDS, and output i is acc = w_r s[i]; acc += w_{r+d} (s[i-d] + s[i+d]), d = 1..r:
//  one lane, one order, every operation rounded on its own -- the result does not depend on the tiling, the grid or alignment.
//  * minmax_kernel: float32 min / max of every map, split over nblk blocks; det_reduce.h's write-through partials and
//    last-arriver fold (min and max do not depend on the order; no floating-point atomics).
//  * POST_PRIOR, after the blur: prior.hip's prior_apply_kernel, when asked for.
//  * POST_MATCH, between the blur and the normalisation: hist_match.hip's launch sequence, when asked for.
//  * apply_kernel: v / mx, or (v - mn) / (mx - mn), correctly rounded, stored back; bytes when asked, whole words where aligned.
#include "p3d_kernels.h"
#include "det_reduce.h"
#include "../../include/p3d_hip.h"
#include <math.h>
#include <algorithm>

// every product and sum below rounds on its own (the header's fmul / fadd): hipcc would otherwise fuse a * b + c
#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr int SEG = 1024;                                  // outputs of one horizontal block: four per thread
constexpr int RMAX = P3D_POST_MAX_RADIUS;
constexpr int LDS_CAP = 65536;
static_assert(P3D_POST_MAX_RADIUS == P3D_BLUR_MAX_RADIUS, "the ABI names the kernels' bound");

// reflect-101 of j into [0, n): one fold is enough for -r <= j <= n - 1 + r with r <= n - 1 (checked by the launcher)
__device__ __forceinline__ int reflect101(int j, int n) { return j < 0 ? -j : (j > n - 1 ? 2 * (n - 1) - j : j); }

__global__ __launch_bounds__(TPB) void blur_h_kernel(const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ taps,
                                                     int r, int H, int W) {
    __shared__ float sw[RMAX + 1];
    __shared__ float row[SEG + 2 * RMAX];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * SEG, seg = min(SEG, W - x0);
    const size_t base = ((size_t)blockIdx.z * H + blockIdx.y) * W;
    for (int d = tid; d <= r; d += TPB) sw[d] = taps[r + d];
    for (int j = tid; j < seg + 2 * r; j += TPB) row[j] = src[base + reflect101(x0 - r + j, W)];
    __syncthreads();
    for (int i = tid; i < seg; i += TPB) {
        const float* c = row + r + i;
        float acc = sw[0] * c[0];
        for (int d = 1; d <= r; ++d) acc = acc + sw[d] * (c[-d] + c[d]);
        dst[base + x0 + i] = acc;
    }
}

// cols: 16, 32 or 64 (a power of two that divides TPB); rows: output rows of one block
__global__ __launch_bounds__(TPB) void blur_v_kernel(const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ taps,
                                                     int r, int H, int W, int cols, int rows) {
    extern __shared__ float lds[];
    float* sw = lds;                                       // [r + 1]
    float* tile = lds + r + 1;                             // [run + 2r][cols]
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * cols, y0 = blockIdx.y * rows;
    const int run = min(rows, H - y0);
    const int cx = tid & (cols - 1), g = tid / cols, G = TPB / cols;
    const size_t base = (size_t)blockIdx.z * H * W;
    const bool inside = x0 + cx < W;
    for (int d = tid; d <= r; d += TPB) sw[d] = taps[r + d];
    for (int j = g; j < run + 2 * r; j += G)
        tile[j * cols + cx] = inside ? src[base + (size_t)reflect101(y0 - r + j, H) * W + x0 + cx] : 0.f;
    __syncthreads();
    if (!inside) return;
    for (int i = g; i < run; i += G) {
        const float* c = tile + (r + i) * cols + cx;
        float acc = sw[0] * c[0];
        for (int d = 1; d <= r; ++d) acc = acc + sw[d] * (c[-d * cols] + c[d * cols]);
        dst[base + (size_t)(y0 + i) * W + x0 + cx] = acc;
    }
}

__device__ __forceinline__ float block_fmin(float v, float* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int o = TPB / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] = fminf(red[tid], red[tid + o]);
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ float block_fmax(float v, float* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int o = TPB / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] = fmaxf(red[tid], red[tid + o]);
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

// grid (nblk, n): block j of map m folds pixels [j * chunk, (j + 1) * chunk)
__global__ __launch_bounds__(TPB) void minmax_kernel(const float* __restrict__ maps, int n_pix, int nblk, float* part, unsigned* counter,
                                                     float* mnmx) {
    __shared__ float red[TPB];
    __shared__ int last;
    const int m = blockIdx.y, tid = threadIdx.x;
    const float* p = maps + (size_t)m * n_pix;
    const int chunk = (n_pix + nblk - 1) / nblk;
    const int i0 = min((long long)blockIdx.x * chunk, (long long)n_pix), i1 = min((long long)i0 + chunk, (long long)n_pix);
    float mn = INFINITY, mx = -INFINITY;
    for (int i = i0 + tid; i < i1; i += TPB) { const float v = p[i]; mn = fminf(mn, v); mx = fmaxf(mx, v); }
    mn = block_fmin(mn, red);
    mx = block_fmax(mx, red);
    float* mp = part + (size_t)m * nblk * 2;
    if (tid < 2) p3d_store_wt(mp, (size_t)blockIdx.x * 2 + tid, tid == 0 ? mn : mx);
    if (!p3d_last_block_wt(counter + m, nblk, &last)) return;
    mn = INFINITY; mx = -INFINITY;
    for (int j = tid; j < nblk; j += TPB) { mn = fminf(mn, mp[(size_t)j * 2]); mx = fmaxf(mx, mp[(size_t)j * 2 + 1]); }
    mn = block_fmin(mn, red);
    mx = block_fmax(mx, red);
    if (tid == 0) { mnmx[m * 2] = mn; mnmx[m * 2 + 1] = mx; }
}

__device__ __forceinline__ float normalised(float v, int norm, float mn, float mx) {
    if (norm == P3D_NORM_MAX) return mx > 0.f ? __fdiv_rn(v, mx) : v;
    if (norm == P3D_NORM_RANGE) return mx > mn ? __fdiv_rn(v - mn, mx - mn) : 0.f;
    return v;
}
// Element j of the launch (map j / n_pix) is byte off + j of u8.  Thread q owns the aligned word of bytes 4q .. 4q+3 (of the
// elements behind them) and stores it whole; the words cut by the launch's ends go byte by byte.  u8 null: floats only, off = 0.
__global__ __launch_bounds__(TPB) void apply_kernel(float* maps, int n, int n_pix, int norm, const float* __restrict__ mnmx, float scale,
                                                    unsigned char* u8, long long off) {
    const long long end = off + (long long)n * n_pix;
    const long long q0 = off >> 2, q1 = (end + 3) >> 2;
    for (long long q = q0 + (long long)blockIdx.x * TPB + threadIdx.x; q < q1; q += (long long)gridDim.x * TPB) {
        const long long b0 = max(q << 2, off), b1 = min((q << 2) + 4, end);
        unsigned v[4] = {0u, 0u, 0u, 0u};
        for (long long b = b0; b < b1; ++b) {
            const long long j = b - off;
            const int m = (int)(j / n_pix);
            float x = maps[j];
            if (norm != P3D_NORM_NONE) {
                x = normalised(x, norm, mnmx[m * 2], mnmx[m * 2 + 1]);
                maps[j] = x;
            }
            if (u8) v[b & 3] = p3d_sat_u8((double)(x * scale));
        }
        if (!u8) continue;
        if (b1 - b0 == 4) {
            reinterpret_cast<unsigned*>(u8)[q] = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
        } else {
            for (long long b = b0; b < b1; ++b) u8[b] = (unsigned char)v[b & 3];
        }
    }
}

bool args_ok(const PostArgs& a) {
    if (a.n < 1 || a.n > 65535 || a.H < 1 || a.W < 1 || (long long)a.H * a.W > INT32_MAX || !a.maps) return false;
    if (a.src && (a.h < 1 || a.w < 1 || a.elem_stride < 1)) return false;
    if (a.r < 0 || a.r > RMAX || a.r > std::min(a.H, a.W) - 1) return false;
    if (a.r > 0 && (!a.tmp || !a.taps || a.tmp == a.maps || a.H > 65535)) return false;
    if (a.norm != P3D_NORM_NONE && a.norm != P3D_NORM_MAX && a.norm != P3D_NORM_RANGE) return false;
    if (a.norm != P3D_NORM_NONE && (!a.part || !a.mnmx || !a.counter || a.nblk != p3d_post_blocks((long long)a.H * a.W))) return false;
    if (a.u8 && ((uintptr_t)a.u8 & 3 || a.u8_off < 0)) return false;
    return true;
}

PriorApplyArgs prior_args(const PostArgs& a) {
    PriorApplyArgs q;
    q.maps = a.maps; q.prior = a.prior; q.n = a.n; q.n_pix = a.H * a.W; q.mode = a.prior_mode; q.nblk = p3d_post_blocks((long long)a.H * a.W);
    q.a = a.prior_a; q.b = a.prior_b;
    return q;
}

}  // namespace

// The widest strip whose rows + 2r staged rows fit the LDS cap, rows = max(2r, 64) where that fits (the halo is then read at most
// once more than the run itself), else what is left.
PostStrip p3d_post_strip(int r) {
    r = std::max(0, std::min(r, RMAX));
    const int cols = r <= 64 ? 64 : r <= 160 ? 32 : 16;
    const int fit = (LDS_CAP - (r + 1) * 4) / (cols * 4) - 2 * r;       // output rows that fit
    const int rows = std::max(1, std::min(fit, std::max(2 * r, 64)));
    return {cols, rows, ((rows + 2 * r) * cols + r + 1) * 4};
}
int p3d_post_blocks(long long n_pix) { return (int)std::max<long long>(1, std::min<long long>((n_pix + 8191) / 8192, 256)); }

bool p3d_post_has(int stage, const PostArgs& a) {
    switch (stage) {
        case POST_RESIZE: return a.src != nullptr;
        case POST_BLUR_H: case POST_BLUR_V: return a.r > 0;
        case POST_PRIOR: return a.prior != nullptr;
        case POST_MATCH: return a.match != nullptr;
        case POST_MINMAX: return a.norm != P3D_NORM_NONE;
        case POST_APPLY: return a.norm != P3D_NORM_NONE || a.u8 != nullptr;
        default: return false;
    }
}

LaunchDesc p3d_post_desc(int stage, const PostArgs& a) {
    const double e = (double)a.n * a.H * a.W, t = 2.0 * a.r + 1.0;
    switch (stage) {
        case POST_RESIZE: return {"resize_f32_kernel", e * 9.0, e * 8.0};
        case POST_BLUR_H: return {"blur_h_kernel", e * (1.5 * t + 0.5), e * 8.0};      // r + 1 products, 2r sums; one read, one write
        case POST_BLUR_V: return {"blur_v_kernel", e * (1.5 * t + 0.5), e * 8.0};
        case POST_PRIOR: return p3d_prior_apply_desc(prior_args(a));
        case POST_MATCH: return {"hist_count_kernel+hist_remap_kernel", e * 14.0, e * 16.0};      // min / max, count, remap: hist_match.hip
        case POST_MINMAX: return {"minmax_kernel", e * 2.0, e * 4.0};
        default: return {"apply_kernel", e * 3.0, e * (a.norm != P3D_NORM_NONE ? 8.0 : 4.0) + (a.u8 ? e : 0.0)};
    }
}

hipError_t p3d_post_launch(int stage, const PostArgs& a, hipStream_t s) {
    if (!args_ok(a) || stage < 0 || stage >= POST_STAGES) return hipErrorInvalidValue;
    if (!p3d_post_has(stage, a)) return hipSuccess;
    const int n_pix = a.H * a.W;
    switch (stage) {
        case POST_RESIZE:
            return p3d_resize_f32(a.src, a.map_stride, a.elem_stride, a.n, a.h, a.w, a.maps, a.H, a.W, s);
        case POST_BLUR_H:
            hipLaunchKernelGGL(blur_h_kernel, dim3((a.W + SEG - 1) / SEG, a.H, a.n), dim3(TPB), 0, s, a.maps, a.tmp, a.taps, a.r, a.H, a.W);
            break;
        case POST_BLUR_V: {
            const PostStrip st = p3d_post_strip(a.r);
            hipLaunchKernelGGL(blur_v_kernel, dim3((a.W + st.cols - 1) / st.cols, (a.H + st.rows - 1) / st.rows, a.n), dim3(TPB),
                               (size_t)st.lds_bytes, s, a.tmp, a.maps, a.taps, a.r, a.H, a.W, st.cols, st.rows);
            break;
        }
        case POST_PRIOR:
            return p3d_prior_apply_launch(prior_args(a), s);
        case POST_MATCH: {
            HistChain c = *a.match;                        // the source: these maps, remapped in place
            c.source.maps = a.maps; c.source.out = a.maps; c.source.n = a.n; c.source.H = a.H; c.source.W = a.W;
            return p3d_hist_chain_launch(c, s);
        }
        case POST_MINMAX:
            hipLaunchKernelGGL(minmax_kernel, dim3(a.nblk, a.n), dim3(TPB), 0, s, a.maps, n_pix, a.nblk, a.part, a.counter, a.mnmx);
            break;
        default: {
            const long long off = a.u8 ? a.u8_off : 0;
            const long long words = ((off + (long long)a.n * n_pix + 3) >> 2) - (off >> 2);
            hipLaunchKernelGGL(apply_kernel, dim3((unsigned)std::min<long long>((words + TPB - 1) / TPB, 65535)), dim3(TPB), 0, s, a.maps,
                               a.n, n_pix, a.norm, a.mnmx, a.scale, a.u8, off);
        }
    }
    return hipGetLastError();
}
