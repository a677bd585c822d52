// Resident training set (p3d_trainset_*; the argument struct in p3d_kernels.h, the contract in include/p3d_hip.h).  The frames, density
// maps and fixation maps of V concatenated videos stay on the device; a batch of B clips, each a (video, start) pair, is cut out
// of the stores into the step's staged x, y and fixation buffers in ONE launch, normalising on the way.  Pure bandwidth: every
// destination element is written by exactly one lane, no atomics, no ordering between blocks, no cross-block state, no LDS.
//
//  * trainset_gather_kernel: blockIdx.y is the clip, blockIdx.z the tensor (x, then y and the fixations where the call names them).
//    A clip's T frames are consecutive in a store, so a clip is ONE contiguous run per tensor, from frame first[blockIdx.y] on.
//      x, TRAINSET_U8   a lane reads 4 pixels = 12 bytes as three dwords and writes their 12 floats as three 16-byte stores:
//                       x[c] = __fdiv_rn(__fsub_rn((float)bgr[2 - c], mean[c]), 255.f), which is mapf_kernel at equal sizes (both
//                       resize weights are 0 there and p - mean + (+-0) keeps p - mean's bits: x - x is +0, never -0)
//      x, TRAINSET_F32  a copy of the bits, 16 bytes per lane (video_gather_kernel's loop)
//      y                a lane reads one dword = 4 bytes and writes 16 bytes: (float)((double)v / 255.0), mapf_density_kernel's
//      fix              a copy of the bytes, 16 per lane
//    The wide forms need the clip's source dword-aligned (16 bytes for the two copies) and its destination 16-byte aligned: the
//    network's case, H * W being a multiple of 16.  Else, and for what is left past the last whole vector, element by element (the
//    hook's misaligned bases, H * W not a multiple of 4).
#include "p3d_kernels.h"
#include <algorithm>

// fsub and fdiv round on their own (there is nothing to contract with; the pragma keeps it so)
#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr long long TS_MAX_BLOCKS = 1024;      // per clip and tensor; the rest is the grid stride

struct TsKernelArgs {
    const void* frames; const unsigned char* density; const unsigned char* fixations;
    float* x; float* y; unsigned char* fix;
    const int* first;
    long long hw; int T;
    int tensor[3];      // what blockIdx.z cuts: 0 x, 1 y, 2 fix
    float m0, m1, m2;
};

__device__ __forceinline__ bool aligned_to(const void* a, unsigned long long n) { return ((unsigned long long)a & (n - 1ull)) == 0; }
__device__ __forceinline__ float norm_u8(unsigned byte, float mean) { return __fdiv_rn(__fsub_rn((float)byte, mean), 255.f); }
__device__ __forceinline__ float density_f32(unsigned byte) { return (float)((double)byte / 255.0); }      // numpy: uint8 / 255. is float64

// byte j of the 12 that three dwords hold
__device__ __forceinline__ unsigned byte_of(unsigned w0, unsigned w1, unsigned w2, int j) {
    const unsigned w = j < 4 ? w0 : j < 8 ? w1 : w2;
    return (w >> (8 * (j & 3))) & 0xffu;
}

// s: n_pix decoded pixels, 3 bytes each in BGR order -> d: n_pix * 3 floats in RGB order
__device__ __forceinline__ void cut_frames_u8(const unsigned char* s, float* d, long long n_pix, float m0, float m1, float m2,
                                              long long tid, long long stride) {
    long long done = 0;
    if (aligned_to(s, 4) && aligned_to(d, 16)) {
        const long long n4 = n_pix >> 2;
        const unsigned* sw = reinterpret_cast<const unsigned*>(s);
        uint4* dv = reinterpret_cast<uint4*>(d);
        for (long long i = tid; i < n4; i += stride) {
            const unsigned w0 = sw[3 * i], w1 = sw[3 * i + 1], w2 = sw[3 * i + 2];
            float f[12];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                f[3 * p + 0] = norm_u8(byte_of(w0, w1, w2, 3 * p + 2), m0);
                f[3 * p + 1] = norm_u8(byte_of(w0, w1, w2, 3 * p + 1), m1);
                f[3 * p + 2] = norm_u8(byte_of(w0, w1, w2, 3 * p + 0), m2);
            }
#pragma unroll
            for (int q = 0; q < 3; ++q)
                dv[3 * i + q] = make_uint4(__float_as_uint(f[4 * q]), __float_as_uint(f[4 * q + 1]), __float_as_uint(f[4 * q + 2]),
                                           __float_as_uint(f[4 * q + 3]));
        }
        done = n4 << 2;
    }
    for (long long p = done + tid; p < n_pix; p += stride) {
        d[3 * p + 0] = norm_u8(s[3 * p + 2], m0);
        d[3 * p + 1] = norm_u8(s[3 * p + 1], m1);
        d[3 * p + 2] = norm_u8(s[3 * p + 0], m2);
    }
}

// a copy of n 4-byte words
__device__ __forceinline__ void cut_words(const unsigned* s, unsigned* d, long long n, long long tid, long long stride) {
    long long done = 0;
    if (aligned_to(s, 16) && aligned_to(d, 16)) {
        const long long n4 = n >> 2;
        for (long long i = tid; i < n4; i += stride) reinterpret_cast<uint4*>(d)[i] = reinterpret_cast<const uint4*>(s)[i];
        done = n4 << 2;
    }
    for (long long i = done + tid; i < n; i += stride) d[i] = s[i];
}

__device__ __forceinline__ void cut_density(const unsigned char* s, float* d, long long n, long long tid, long long stride) {
    long long done = 0;
    if (aligned_to(s, 4) && aligned_to(d, 16)) {
        const long long n4 = n >> 2;
        for (long long i = tid; i < n4; i += stride) {
            const unsigned w = reinterpret_cast<const unsigned*>(s)[i];
            reinterpret_cast<uint4*>(d)[i] = make_uint4(__float_as_uint(density_f32(w & 0xffu)), __float_as_uint(density_f32((w >> 8) & 0xffu)),
                                                        __float_as_uint(density_f32((w >> 16) & 0xffu)), __float_as_uint(density_f32(w >> 24)));
        }
        done = n4 << 2;
    }
    for (long long i = done + tid; i < n; i += stride) d[i] = density_f32(s[i]);
}

__device__ __forceinline__ void cut_bytes(const unsigned char* s, unsigned char* d, long long n, long long tid, long long stride) {
    long long done = 0;
    if (aligned_to(s, 16) && aligned_to(d, 16)) {
        const long long n16 = n >> 4;
        for (long long i = tid; i < n16; i += stride) reinterpret_cast<uint4*>(d)[i] = reinterpret_cast<const uint4*>(s)[i];
        done = n16 << 4;
    }
    for (long long i = done + tid; i < n; i += stride) d[i] = s[i];
}

template <int FORMAT>
__global__ __launch_bounds__(TPB) void trainset_gather_kernel(TsKernelArgs a) {
    const long long clip = (long long)a.T * a.hw;                       // pixels of one clip
    const long long src = (long long)a.first[blockIdx.y] * a.hw;        // the clip's first pixel in a store
    const long long dst = (long long)blockIdx.y * clip;
    const long long stride = (long long)gridDim.x * TPB, tid = (long long)blockIdx.x * TPB + threadIdx.x;
    const int tensor = a.tensor[blockIdx.z];
    if (tensor == 0) {
        if (FORMAT == TRAINSET_U8)
            cut_frames_u8(static_cast<const unsigned char*>(a.frames) + src * 3, a.x + dst * 3, clip, a.m0, a.m1, a.m2, tid, stride);
        else
            cut_words(static_cast<const unsigned*>(a.frames) + src * 3, reinterpret_cast<unsigned*>(a.x) + dst * 3, clip * 3, tid, stride);
    } else if (tensor == 1) {
        cut_density(a.density + src, a.y + dst, clip, tid, stride);
    } else {
        cut_bytes(a.fixations + src, a.fix + dst, clip, tid, stride);
    }
}

unsigned grid_x(long long work) { return (unsigned)std::min<long long>(std::max<long long>((work + TPB - 1) / TPB, 1), TS_MAX_BLOCKS); }

bool gather_ok(const TrainsetGatherArgs& a) {
    if (a.format != TRAINSET_U8 && a.format != TRAINSET_F32) return false;
    if (!a.frames || !a.x || !a.first || !a.first_host || !a.video_host || !a.start_host || !a.frames_host) return false;
    if ((a.y && !a.density) || (a.fix && !a.fixations)) return false;
    if (a.B < 1 || a.B > 65535 || a.T < 1 || a.hw < 1 || a.n_videos < 1) return false;
    for (int k = 0; k < a.B; ++k) {      // no clip may leave its video: the gather trusts the table
        const int v = a.video_host[k];
        if (v < 0 || v >= a.n_videos) return false;
        if (a.start_host[k] < 0 || a.start_host[k] > a.frames_host[v] - a.T) return false;
        long long base = 0;
        for (int u = 0; u < v; ++u) base += a.frames_host[u];
        if ((long long)a.first_host[k] != base + a.start_host[k]) return false;
    }
    return true;
}

}  // namespace

LaunchDesc p3d_trainset_gather_desc(const TrainsetGatherArgs& a) {
    const double px = (double)a.B * a.T * (double)a.hw;
    const double fl = (a.format == TRAINSET_U8 ? 6.0 : 0.0) + (a.y ? 1.0 : 0.0);
    const double by = (a.format == TRAINSET_U8 ? 15.0 : 24.0) + (a.y ? 5.0 : 0.0) + (a.fix ? 2.0 : 0.0);
    return {a.format == TRAINSET_U8 ? "trainset_gather_kernel<0>" : "trainset_gather_kernel<1>", fl * px, by * px};
}

hipError_t p3d_trainset_gather(const TrainsetGatherArgs& a, hipStream_t s) {
    if (!gather_ok(a)) return hipErrorInvalidValue;
    TsKernelArgs k;
    k.frames = a.frames; k.density = a.density; k.fixations = a.fixations;
    k.x = a.x; k.y = a.y; k.fix = a.fix; k.first = a.first; k.hw = a.hw; k.T = a.T;
    k.m0 = a.mean[0]; k.m1 = a.mean[1]; k.m2 = a.mean[2];
    int nz = 0;
    k.tensor[0] = k.tensor[1] = k.tensor[2] = 0;
    k.tensor[nz++] = 0;
    if (a.y) k.tensor[nz++] = 1;
    if (a.fix) k.tensor[nz++] = 2;
    const long long clip = (long long)a.T * a.hw;
    // the widest tensor sizes the grid: 4 pixels per lane (U8 frames, density), or 16 bytes of floats
    const long long work = a.format == TRAINSET_U8 ? (clip + 3) / 4 : (clip * 3 + 3) / 4;
    const dim3 grid(grid_x(work), a.B, nz);
    if (a.format == TRAINSET_U8) hipLaunchKernelGGL(trainset_gather_kernel<TRAINSET_U8>, grid, dim3(TPB), 0, s, k);
    else hipLaunchKernelGGL(trainset_gather_kernel<TRAINSET_F32>, grid, dim3(TPB), 0, s, k);
    return hipGetLastError();
}
