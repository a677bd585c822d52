// Clip augmentation of the staged inputs of a train step (p3d_set_augment; AugArgs in p3d_kernels.h, the contract in
// include/p3d_hip.h).  One row of decisions per clip -- crop window, flip, temporal reversal, contrast and brightness -- reaches the
// kernels as a table in device memory and is applied alike to x [B,T,H,W,3], y [B,T,H,W] and the fixation bytes [B,T,H,W], so the
// maps stay registered to the frames.  Crop-and-resize, flip and reversal compose into ONE gather: destination (t, h, w) reads the
// window's taps of frame T-1-t (reversed) for column W-1-w (flipped), and every destination element is written once.
//
//  * augment_f32_kernel<C>: x (C = 3, with the photometric step) and y (C = 1).  blockIdx.y is the clip; consecutive lanes take
//    consecutive destination floats of a row (a flipped row reads a contiguous segment backwards).  The resize is
//    resize_f32_kernel's (metrics_full.hip): cv2.INTER_LINEAR's coordinates in double, float32 weights, horizontal pass then
//    vertical, no contraction -- bit-exact to oracle/dataflow.py:resize_linear on the cropped window.  A window equal to the frame
//    reads one tap and does no arithmetic; a == 1 and b == 0 does none either, so NaN, inf and -0 pass through.
//  * augment_fix_kernel: the fixation bytes by fixations_to_grid's law on the window (a gather: ch <= H, so at most one source row
//    and column per cell); four cells per lane stored as one word where the clip's destination is 4-byte aligned.
//  * A clip whose decisions are all neutral is a block-uniform branch to a plain copy, 16 bytes per lane where the clip's source
//    and destination are 16-byte aligned, else element by element (the hook's misaligned bases).
// No atomics, no cross-block state.  Memory-bound: each element is read and written once (four taps of a cropped clip mostly hit
// the same lines).
#include "p3d_kernels.h"
#include <math.h>
#include <algorithm>

// the resize and fadd(fmul(x, a), b) round every operation on its own, like OpenCV's generic path and the numpy replay
#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr unsigned AUG_MAX_BLOCKS = 1024;      // per clip; the rest is the grid stride

// cv2 (resize.cpp, resizeGeneric_), as metrics_full.hip's lin_coef_rn: fx = (float)((d + 0.5) * scale - 0.5), floor, weight 0 at
// a clamped border; scale = src / dst in double
__device__ __forceinline__ void lin_coef_rn(int d, double scale, int extent, int& s0, int& s1, float& w1) {
    float fx = (float)(((double)d + 0.5) * scale - 0.5);
    int sx = (int)floorf(fx);
    fx -= (float)sx;
    if (sx < 0) { sx = 0; fx = 0.f; }
    if (sx >= extent - 1) { sx = extent - 1; fx = 0.f; }
    s0 = sx; s1 = min(sx + 1, extent - 1); w1 = fx;
}

__device__ __forceinline__ bool aligned16(const void* a, const void* b) {
    return (((unsigned long long)a | (unsigned long long)b) & 15ull) == 0;
}

template <int C>
__global__ __launch_bounds__(TPB) void augment_f32_kernel(const float* src, float* dst, const P3dAugClip* tab, int T, int H, int W,
                                                          int with_photo) {
    const P3dAugClip k = tab[blockIdx.y];
    const int n = T * H * W * C;                                   // one clip; <= 2^30 (p3d_augment_launch)
    const float* s = src + (long long)blockIdx.y * n;
    float* d = dst + (long long)blockIdx.y * n;
    const bool full = k.ch == H && k.cw == W;
    const bool photo = with_photo && !(k.a == 1.f && k.b == 0.f);
    const int stride = (int)gridDim.x * TPB, tid = (int)blockIdx.x * TPB + (int)threadIdx.x;
    if (full && !k.flip && !k.reverse && !photo) {                 // the neutral clip: a copy of the bits
        const unsigned* su = reinterpret_cast<const unsigned*>(s);
        unsigned* du = reinterpret_cast<unsigned*>(d);
        int done = 0;
        if (aligned16(s, d)) {
            const int n4 = n >> 2;
            for (int i = tid; i < n4; i += stride) reinterpret_cast<uint4*>(du)[i] = reinterpret_cast<const uint4*>(su)[i];
            done = n4 << 2;
        }
        for (int i = done + tid; i < n; i += stride) du[i] = su[i];
        return;
    }
    const double sx = (double)k.cw / W, sy = (double)k.ch / H;
    const int frame = H * W * C;
    for (int i = tid; i < n; i += stride) {
        const int c = i % C, pix = i / C;
        const int w = pix % W, r = pix / W;
        const int h = r % H, t = r / H;
        const int ws = k.flip ? W - 1 - w : w, ts = k.reverse ? T - 1 - t : t;
        const float* f = s + (long long)ts * frame + c;
        float v;
        if (full) {
            v = f[(h * W + ws) * C];
        } else {
            int x0, x1, y0, y1; float wx, wy;
            lin_coef_rn(ws, sx, k.cw, x0, x1, wx);
            lin_coef_rn(h, sy, k.ch, y0, y1, wy);
            const float* r0p = f + (long long)(k.y0 + y0) * W * C;
            const float* r1p = f + (long long)(k.y0 + y1) * W * C;
            const int c0 = (k.x0 + x0) * C, c1 = (k.x0 + x1) * C;
            const float p00 = r0p[c0], p01 = r0p[c1], p10 = r1p[c0], p11 = r1p[c1];
            const float ax = 1.f - wx, ay = 1.f - wy;
            const float r0 = p00 * ax + p01 * wx;
            const float r1 = p10 * ax + p11 * wx;
            v = r0 * ay + r1 * wy;
        }
        if (photo) {
            v = v * k.a;
            v = v + k.b;
        }
        d[i] = v;
    }
}

// destination byte i of a clip that is not neutral; s = the clip's source bytes
__device__ __forceinline__ unsigned aug_fix_cell(const unsigned char* s, const P3dAugClip& k, bool full, int T, int H, int W, int i) {
    const int w = i % W, r = i / W;
    const int h = r % H, t = r / H;
    const int ws = k.flip ? W - 1 - w : w, ts = k.reverse ? T - 1 - t : t;
    const unsigned char* f = s + (long long)ts * H * W;
    if (full) return f[h * W + ws];
    // the one window row rr with rr * H / ch == h, if there is one: the smallest rr with rr * H >= h * ch
    const int rr = (h * k.ch + H - 1) / H, cc = (ws * k.cw + W - 1) / W;
    if (rr >= k.ch || rr * H / k.ch != h || cc >= k.cw || cc * W / k.cw != ws) return 0u;
    return f[(k.y0 + rr) * W + k.x0 + cc] >= 128 ? 255u : 0u;
}

__global__ __launch_bounds__(TPB) void augment_fix_kernel(const unsigned char* src, unsigned char* dst, const P3dAugClip* tab, int T, int H,
                                                          int W) {
    const P3dAugClip k = tab[blockIdx.y];
    const int n = T * H * W;
    const unsigned char* s = src + (long long)blockIdx.y * n;
    unsigned char* d = dst + (long long)blockIdx.y * n;
    const bool full = k.ch == H && k.cw == W;
    const int stride = (int)gridDim.x * TPB, tid = (int)blockIdx.x * TPB + (int)threadIdx.x;
    if (full && !k.flip && !k.reverse) {                           // the neutral clip: a copy of the bytes
        int done = 0;
        if (aligned16(s, d)) {
            const int n16 = n >> 4;
            for (int i = tid; i < n16; i += stride) reinterpret_cast<uint4*>(d)[i] = reinterpret_cast<const uint4*>(s)[i];
            done = n16 << 4;
        }
        for (int i = done + tid; i < n; i += stride) d[i] = s[i];
        return;
    }
    int done = 0;
    if (((unsigned long long)d & 3ull) == 0) {                     // four cells per lane, stored as one word
        const int n4 = n >> 2;
        for (int i = tid; i < n4; i += stride) {
            const int e = i << 2;
            const unsigned v = aug_fix_cell(s, k, full, T, H, W, e) | (aug_fix_cell(s, k, full, T, H, W, e + 1) << 8) |
                               (aug_fix_cell(s, k, full, T, H, W, e + 2) << 16) | (aug_fix_cell(s, k, full, T, H, W, e + 3) << 24);
            reinterpret_cast<unsigned*>(d)[i] = v;
        }
        done = n4 << 2;
    }
    for (int i = done + tid; i < n; i += stride) d[i] = (unsigned char)aug_fix_cell(s, k, full, T, H, W, i);
}

unsigned grid_x(long long work) { return (unsigned)std::min<long long>((work + TPB - 1) / TPB, AUG_MAX_BLOCKS); }

long long clip_elems(const AugArgs& a) { return (long long)a.T * a.H * a.W; }

bool args_ok(const AugArgs& a) {
    if (!a.x || !a.y || !a.x_out || !a.y_out || !a.tab || !a.tab_host) return false;
    if (a.fix && !a.fix_out) return false;
    if (a.x == a.x_out || a.y == a.y_out || (a.fix && a.fix == a.fix_out)) return false;
    if (a.B < 1 || a.B > 65535 || a.T < 1 || a.H < 1 || a.W < 1 || a.H > 32768 || a.W > 32768) return false;
    if (clip_elems(a) * 3 > (1ll << 30)) return false;
    for (int b = 0; b < a.B; ++b) {      // no window may leave the frame: the gathers trust the table
        const P3dAugClip& k = a.tab_host[b];
        if (k.ch < 1 || k.cw < 1 || k.y0 < 0 || k.x0 < 0 || k.ch > a.H || k.cw > a.W || k.y0 > a.H - k.ch || k.x0 > a.W - k.cw) return false;
    }
    return true;
}

}  // namespace

LaunchDesc p3d_augment_desc(int stage, const AugArgs& a) {
    // every element read and written once (the taps of a resized clip share lines); per resized float: two coordinate rules and
    // the six products and three sums of the two passes, and on x a product and a sum more
    const double e = (double)a.B * (double)clip_elems(a);
    if (stage == AUG_X) return {"augment_f32_kernel<3>", 3.0 * e * 11.0, 3.0 * e * 8.0};
    if (stage == AUG_Y) return {"augment_f32_kernel<1>", e * 9.0, e * 8.0};
    return {"augment_fix_kernel", 0.0, e * 2.0};
}

hipError_t p3d_augment_launch(int stage, const AugArgs& a, hipStream_t s) {
    if (!args_ok(a) || stage < AUG_X || stage > AUG_FIX || (stage == AUG_FIX && !a.fix)) return hipErrorInvalidValue;
    const long long e = clip_elems(a);
    if (stage == AUG_X)
        hipLaunchKernelGGL(augment_f32_kernel<3>, dim3(grid_x(e * 3), a.B), dim3(TPB), 0, s, a.x, a.x_out, a.tab, a.T, a.H, a.W, 1);
    else if (stage == AUG_Y)
        hipLaunchKernelGGL(augment_f32_kernel<1>, dim3(grid_x(e), a.B), dim3(TPB), 0, s, a.y, a.y_out, a.tab, a.T, a.H, a.W, 0);
    else
        hipLaunchKernelGGL(augment_fix_kernel, dim3(grid_x((e + 3) / 4), a.B), dim3(TPB), 0, s, a.fix, a.fix_out, a.tab, a.T, a.H, a.W);
    return hipGetLastError();
}
