// Resident video inference (p3d_video_*; the argument structs in p3d_kernels.h, the contract in include/p3d_hip.h).  A video's
// normalised frames [F][H][W][3] and its saliency maps [F][H][W] stay on the device; windows are cut out of the frame store into
// the staged input, and a batch's predictions are folded into the map store, one launch each way.  Pure bandwidth kernels: every
// element is read and written once, no arithmetic but MEAN's one add per contribution and the read-out's one division.
//
//  * video_gather_kernel: blockIdx.y is the clip.  A window's T frames are consecutive in the store, so a clip is ONE contiguous
//    run of T * frame_elems floats; consecutive lanes take consecutive floats, 16 bytes per lane where the clip's source and
//    destination are 16-byte aligned (the network's case: H and W are multiples of 16), else element by element (the hook's
//    misaligned bases, and whatever is left past the last whole 16 bytes).  A copy of the bits.
//  * video_gather_slots_kernel (p3d_video_predict_shots): blockIdx.y is a slot of the call's table frames [B * T].  A window that
//    reflects inside a short shot is not one run of the store, so every slot is its own contiguous run of frame_elems floats, copied
//    as the clip above is: 16 bytes per lane where that slot's source and destination are 16-byte aligned, else element by element.
//  * video_scatter_kernel<MODE>: blockIdx.y is a destination frame of the call's table (P3dVideoDst), and every destination element
//    is written by exactly one lane, which walks the frame's contributing maps in the table's order (ascending window).  NEWEST
//    copies the first contributor's bits; MEAN starts from them (count 0 before the call) or from the stored sum and adds the
//    rest in float32, one rounding per add.  The prediction is read with its element stride ld; 16 bytes per lane only where
//    ld == 1, hw is a multiple of 4 and both bases are 16-byte aligned.  Lane 0 of the frame's first block stores the new count.
//  * video_mean_kernel: out = sum / (float)count, correctly rounded, per element; a count of 1 copies the bits.
// No atomics, no ordering between blocks, no cross-block state.
#include "p3d_kernels.h"
#include <algorithm>

// fadd and fdiv round on their own (there is nothing to contract with; the pragma keeps it so)
#pragma clang fp contract(off)

namespace {

constexpr int TPB = 256;
constexpr long long VID_MAX_BLOCKS = 1024;      // per clip / frame; the rest is the grid stride

__device__ __forceinline__ bool aligned16(const void* a, const void* b) {
    return (((unsigned long long)a | (unsigned long long)b) & 15ull) == 0;
}

__global__ __launch_bounds__(TPB) void video_gather_kernel(const float* store, float* x, const int* starts, long long frame_elems,
                                                           long long clip_elems) {
    const unsigned* s = reinterpret_cast<const unsigned*>(store + (long long)starts[blockIdx.y] * frame_elems);
    unsigned* d = reinterpret_cast<unsigned*>(x + (long long)blockIdx.y * clip_elems);
    const long long stride = (long long)gridDim.x * TPB, tid = (long long)blockIdx.x * TPB + threadIdx.x;
    long long done = 0;
    if (aligned16(s, d)) {
        const long long n4 = clip_elems >> 2;
        for (long long i = tid; i < n4; i += stride) reinterpret_cast<uint4*>(d)[i] = reinterpret_cast<const uint4*>(s)[i];
        done = n4 << 2;
    }
    for (long long i = done + tid; i < clip_elems; i += stride) d[i] = s[i];
}

__global__ __launch_bounds__(TPB) void video_gather_slots_kernel(const float* store, float* x, const int* frames, long long frame_elems) {
    const unsigned* s = reinterpret_cast<const unsigned*>(store + (long long)frames[blockIdx.y] * frame_elems);
    unsigned* d = reinterpret_cast<unsigned*>(x + (long long)blockIdx.y * frame_elems);
    const long long stride = (long long)gridDim.x * TPB, tid = (long long)blockIdx.x * TPB + threadIdx.x;
    long long done = 0;
    if (aligned16(s, d)) {
        const long long n4 = frame_elems >> 2;
        for (long long i = tid; i < n4; i += stride) reinterpret_cast<uint4*>(d)[i] = reinterpret_cast<const uint4*>(s)[i];
        done = n4 << 2;
    }
    for (long long i = done + tid; i < frame_elems; i += stride) d[i] = s[i];
}

template <int MODE>
__global__ __launch_bounds__(TPB) void video_scatter_kernel(const float* pred, int ld, long long hw, float* store, int32_t* count,
                                                            const P3dVideoDst* dst, const int* src) {
    const P3dVideoDst f = dst[blockIdx.y];
    const int* c = src + f.first;
    const int nc = MODE == VIDEO_MEAN ? f.n : 1;
    unsigned* o = reinterpret_cast<unsigned*>(store + (long long)f.frame * hw);
    const long long stride = (long long)gridDim.x * TPB, tid = (long long)blockIdx.x * TPB + threadIdx.x;
    if (ld == 1 && (hw & 3) == 0 && aligned16(pred, store)) {
        const long long n4 = hw >> 2;
        for (long long i = tid; i < n4; i += stride) {
            int j = 0;
            uint4 a;
            if (MODE == VIDEO_MEAN && f.before != 0) a = reinterpret_cast<const uint4*>(o)[i];
            else a = reinterpret_cast<const uint4*>(pred + (long long)c[j++] * hw)[i];
            for (; j < nc; ++j) {
                const uint4 p = reinterpret_cast<const uint4*>(pred + (long long)c[j] * hw)[i];
                a.x = __float_as_uint(__uint_as_float(a.x) + __uint_as_float(p.x));
                a.y = __float_as_uint(__uint_as_float(a.y) + __uint_as_float(p.y));
                a.z = __float_as_uint(__uint_as_float(a.z) + __uint_as_float(p.z));
                a.w = __float_as_uint(__uint_as_float(a.w) + __uint_as_float(p.w));
            }
            reinterpret_cast<uint4*>(o)[i] = a;
        }
    } else {
        const unsigned* pu = reinterpret_cast<const unsigned*>(pred);
        for (long long i = tid; i < hw; i += stride) {
            int j = 0;
            unsigned a;
            if (MODE == VIDEO_MEAN && f.before != 0) a = o[i];
            else a = pu[((long long)c[j++] * hw + i) * ld];
            for (; j < nc; ++j) a = __float_as_uint(__uint_as_float(a) + __uint_as_float(pu[((long long)c[j] * hw + i) * ld]));
            o[i] = a;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) count[f.frame] = MODE == VIDEO_MEAN ? f.before + f.n : 1;
}

__global__ __launch_bounds__(TPB) void video_mean_kernel(const float* sum, const int32_t* count, float* out, long long hw) {
    const int cnt = count[blockIdx.y];
    const float div = (float)cnt;
    const unsigned* s = reinterpret_cast<const unsigned*>(sum + (long long)blockIdx.y * hw);
    unsigned* o = reinterpret_cast<unsigned*>(out + (long long)blockIdx.y * hw);
    const long long stride = (long long)gridDim.x * TPB, tid = (long long)blockIdx.x * TPB + threadIdx.x;
    long long done = 0;
    if (aligned16(s, o)) {
        const long long n4 = hw >> 2;
        for (long long i = tid; i < n4; i += stride) {
            uint4 a = reinterpret_cast<const uint4*>(s)[i];
            if (cnt != 1) {
                a.x = __float_as_uint(__fdiv_rn(__uint_as_float(a.x), div));
                a.y = __float_as_uint(__fdiv_rn(__uint_as_float(a.y), div));
                a.z = __float_as_uint(__fdiv_rn(__uint_as_float(a.z), div));
                a.w = __float_as_uint(__fdiv_rn(__uint_as_float(a.w), div));
            }
            reinterpret_cast<uint4*>(o)[i] = a;
        }
        done = n4 << 2;
    }
    for (long long i = done + tid; i < hw; i += stride) o[i] = cnt != 1 ? __float_as_uint(__fdiv_rn(__uint_as_float(s[i]), div)) : s[i];
}

unsigned grid_x(long long work) { return (unsigned)std::min<long long>(std::max<long long>((work + TPB - 1) / TPB, 1), VID_MAX_BLOCKS); }

bool gather_ok(const VideoGatherArgs& a) {
    if (!a.store || !a.x || !a.starts || !a.starts_host) return false;
    if (a.B < 1 || a.B > 65535 || a.T < 1 || a.F < a.T || a.frame_elems < 1) return false;
    for (int b = 0; b < a.B; ++b)      // no window may leave the store: the gather trusts the table
        if (a.starts_host[b] < 0 || a.starts_host[b] > a.F - a.T) return false;
    return true;
}

bool gather_slots_ok(const VideoGatherSlotsArgs& a) {
    if (!a.store || !a.x || !a.frames || !a.frames_host) return false;
    if (a.B < 1 || a.T < 1 || (long long)a.B * a.T > 65535 || a.F < 1 || a.frame_elems < 1) return false;
    for (int i = 0; i < a.B * a.T; ++i)      // no slot may leave the store: the gather trusts the table
        if (a.frames_host[i] < 0 || a.frames_host[i] >= a.F) return false;
    return true;
}

bool scatter_ok(const VideoScatterArgs& a) {
    if (!a.pred || !a.store || !a.count || !a.dst || !a.src || !a.dst_host || !a.src_host) return false;
    if (a.mode != VIDEO_NEWEST && a.mode != VIDEO_MEAN) return false;
    if (a.ld < 1 || a.hw < 1 || a.F < 1 || a.maps < 1 || a.ndst < 1 || a.ndst > 65535 || a.nsrc < 1) return false;
    for (int i = 0; i < a.ndst; ++i) {      // every table row stays inside the stores: the scatter trusts the table
        const P3dVideoDst& d = a.dst_host[i];
        if (d.frame < 0 || d.frame >= a.F || d.before < 0 || d.n < 1 || d.first < 0 || d.first > a.nsrc - d.n) return false;
        if (i > 0 && d.frame <= a.dst_host[i - 1].frame) return false;      // one writer per frame
    }
    for (int i = 0; i < a.nsrc; ++i)
        if (a.src_host[i] < 0 || a.src_host[i] >= a.maps) return false;
    return true;
}

}  // namespace

LaunchDesc p3d_video_gather_desc(const VideoGatherArgs& a) {
    return {"video_gather_kernel", 0.0, (double)a.B * a.T * (double)a.frame_elems * 8.0};
}

hipError_t p3d_video_gather(const VideoGatherArgs& a, hipStream_t s) {
    if (!gather_ok(a)) return hipErrorInvalidValue;
    const long long clip = (long long)a.T * a.frame_elems;
    hipLaunchKernelGGL(video_gather_kernel, dim3(grid_x((clip + 3) / 4), a.B), dim3(TPB), 0, s, a.store, a.x, a.starts, a.frame_elems, clip);
    return hipGetLastError();
}

LaunchDesc p3d_video_gather_slots_desc(const VideoGatherSlotsArgs& a) {
    return {"video_gather_slots_kernel", 0.0, (double)a.B * a.T * (double)a.frame_elems * 8.0};
}

hipError_t p3d_video_gather_slots(const VideoGatherSlotsArgs& a, hipStream_t s) {
    if (!gather_slots_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(video_gather_slots_kernel, dim3(grid_x((a.frame_elems + 3) / 4), a.B * a.T), dim3(TPB), 0, s, a.store, a.x, a.frames,
                       a.frame_elems);
    return hipGetLastError();
}

LaunchDesc p3d_video_scatter_desc(const VideoScatterArgs& a) {
    // per destination frame: its contributors read, the frame written, and under MEAN the stored sum read and an add per contributor
    double reads = 0.0, adds = 0.0;
    for (int i = 0; i < a.ndst && a.dst_host; ++i) {
        const P3dVideoDst& d = a.dst_host[i];
        const int nc = a.mode == VIDEO_MEAN ? d.n : 1;
        reads += nc + (a.mode == VIDEO_MEAN && d.before != 0 ? 1 : 0);
        adds += nc - (a.mode == VIDEO_MEAN && d.before != 0 ? 0 : 1);
    }
    return {a.mode == VIDEO_MEAN ? "video_scatter_kernel<1>" : "video_scatter_kernel<0>", adds * (double)a.hw,
            (reads + (double)a.ndst) * (double)a.hw * 4.0};
}

hipError_t p3d_video_scatter(const VideoScatterArgs& a, hipStream_t s) {
    if (!scatter_ok(a)) return hipErrorInvalidValue;
    const bool vec = a.ld == 1 && (a.hw & 3) == 0;
    const dim3 grid(grid_x(vec ? a.hw / 4 : a.hw), a.ndst);
    if (a.mode == VIDEO_MEAN)
        hipLaunchKernelGGL(video_scatter_kernel<VIDEO_MEAN>, grid, dim3(TPB), 0, s, a.pred, a.ld, a.hw, a.store, a.count, a.dst, a.src);
    else
        hipLaunchKernelGGL(video_scatter_kernel<VIDEO_NEWEST>, grid, dim3(TPB), 0, s, a.pred, a.ld, a.hw, a.store, a.count, a.dst, a.src);
    return hipGetLastError();
}

LaunchDesc p3d_video_mean_desc(const VideoMeanArgs& a) { return {"video_mean_kernel", (double)a.n * (double)a.hw, (double)a.n * (double)a.hw * 8.0}; }

hipError_t p3d_video_mean(const VideoMeanArgs& a, hipStream_t s) {
    if (!a.sum || !a.count || !a.out || a.sum == a.out || a.n < 1 || a.n > 65535 || a.hw < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(video_mean_kernel, dim3(grid_x((a.hw + 3) / 4), a.n), dim3(TPB), 0, s, a.sum, a.count, a.out, a.hw);
    return hipGetLastError();
}
