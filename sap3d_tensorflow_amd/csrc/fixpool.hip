// Fixation pool and shuffled AUC's sampling on the device (p3d_fixpool_*, p3d_eval_shuffled_*; FixPackArgs / FixUnionArgs /
// FixSelectArgs in p3d_kernels.h, the law in include/p3d_hip.h): the fixation maps of a test set are kept as one bit per pixel,
// the union of M of them is an OR of words, and np.nonzero(other)[0][rank] is a rank-select over popcounts.  Integer work only:
// no sum here has an order to pin.
//
//  * fix_pack_kernel: grid (blocks, maps).  A map whose first byte is 16-byte aligned takes the wide path: a lane loads 16 bytes,
//    gathers their top bits into 16 predicates (one multiply per dword), and four neighbouring lanes OR their quarters of a
//    word together with two cross-lane exchanges; the lane of the low quarter stores the word.  Any other map (map i of a call
//    starts at byte i * H * W) takes the element path: a wave per word, a byte per lane, the word is the wave's 64-bit ballot
//    and lane 0 stores it.  Either way a word has one writer and is stored whole by a plain vector store; bytes past the end
//    of the map are never read and count as 0.
//  * fix_union_kernel: grid (scan blocks, B), a thread per word.  OR over the row's M pool slots, popcount, an exclusive scan of
//    the block's 256 counts (wave scans by lane exchange, the four wave totals through LDS), the block's total stored
//    write-through; the last arriving block of the map scans the block totals in place and stores the map's total.
//  * fix_select_kernel: grid (blocks, B), a thread per rank.  Two bisections (the scan blocks' sums, then the words' prefixes
//    inside the block), then the r-th set bit of one word by six popcounts of its lower halves.
#include "p3d_kernels.h"
#include "det_reduce.h"
#include "../../include/p3d_hip.h"
#include <algorithm>

namespace {

constexpr int TPB = 256;
static_assert(P3D_FIX_SCAN_WORDS == TPB && P3D_FIX_SCAN_BLOCK == TPB, "a thread per word of a scan block; the ABI names the seam");

// the top bits of the four bytes of w as bits 0 .. 3: byte i's flag sits at bit 8i and the products move it to bit 24 + i
__device__ __forceinline__ unsigned top_bits4(unsigned w) { return (((w >> 7) & 0x01010101u) * 0x01020408u) >> 24; }

__global__ __launch_bounds__(TPB) void fix_pack_kernel(FixPackArgs a) {
    const long long nw = p3d_fix_words(a.n_pix);
    const unsigned char* src = a.maps + (long long)blockIdx.y * a.n_pix;
    unsigned long long* dst = a.words + (long long)blockIdx.y * nw;
    const int lane = threadIdx.x & 63;
    if (((uintptr_t)src & 15) == 0) {                      // block-uniform
        const long long nt = nw * 4;                       // quarter words; TPB is a multiple of 4: a word's quarters share a wave
        for (long long t0 = (long long)blockIdx.x * TPB; t0 < nt; t0 += (long long)gridDim.x * TPB) {
            const long long t = t0 + threadIdx.x, p = t * 16;
            unsigned bits = 0u;
            if (p + 16 <= a.n_pix) {
                const uint4 v = *reinterpret_cast<const uint4*>(src + p);
                bits = top_bits4(v.x) | (top_bits4(v.y) << 4) | (top_bits4(v.z) << 8) | (top_bits4(v.w) << 12);
            } else {
                for (int j = 0; j < 16 && p + j < a.n_pix; ++j) bits |= (src[p + j] >= 128 ? 1u : 0u) << j;
            }
            unsigned long long w = (unsigned long long)bits << (16 * (lane & 3));
            w |= __shfl_xor(w, 1);
            w |= __shfl_xor(w, 2);
            if (t < nt && (lane & 3) == 0) dst[t >> 2] = w;
        }
    } else {
        const long long waves = (long long)gridDim.x * (TPB / 64);
        for (long long k = (long long)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6); k < nw; k += waves) {      // wave-uniform
            const long long p = k * 64 + lane;
            const unsigned long long w = __ballot(p < a.n_pix && src[p] >= 128);
            if (lane == 0) dst[k] = w;
        }
    }
}

__global__ __launch_bounds__(TPB) void fix_union_kernel(FixUnionArgs a) {
    __shared__ unsigned wtot[TPB / 64], offs[TPB + 1];
    __shared__ int last;
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long k = (long long)blockIdx.x * TPB + tid;
    unsigned long long w = 0ull;
    if (k < a.nw)
        for (int m = 0; m < a.M; ++m) w |= a.pool[(long long)a.ids[b * a.M + m] * a.nw + k];
    const unsigned c = (unsigned)__popcll(w);
    unsigned incl = c;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    unsigned before = 0u, total = 0u;
    for (int v = 0; v < TPB / 64; ++v) { if (v < wave) before += wtot[v]; total += wtot[v]; }
    if (k < a.nw) {
        a.uni[(long long)b * a.nw + k] = w;
        a.prefix[(long long)b * a.nw + k] = before + incl - c;
    }
    unsigned* bs = a.bsum + (size_t)b * a.nsb;
    if (tid == 0) p3d_store_wt(reinterpret_cast<float*>(bs), blockIdx.x, __uint_as_float(total));
    if (!p3d_last_block_wt(a.counter + b, a.nsb, &last)) return;
    // the block sums -> their exclusive scan, in place: thread chunks, then the chunks' offsets
    const int c2 = (a.nsb + TPB - 1) / TPB;
    const int j0 = min(a.nsb, tid * c2), j1 = min(a.nsb, j0 + c2);
    unsigned run = 0u;
    for (int j = j0; j < j1; ++j) run += bs[j];
    offs[tid + 1] = run;
    if (tid == 0) offs[0] = 0u;
    __syncthreads();
    if (tid == 0) for (int t = 0; t < TPB; ++t) offs[t + 1] += offs[t];
    __syncthreads();
    run = offs[tid];
    for (int j = j0; j < j1; ++j) { const unsigned v = bs[j]; bs[j] = run; run += v; }
    if (tid == 0) a.n_other[b] = offs[TPB];
}

__global__ __launch_bounds__(TPB) void fix_select_kernel(FixSelectArgs a) {
    const int b = blockIdx.y;
    const long long n = (long long)a.n_rows[b] * a.n_rep;
    const int* ranks = a.ranks + a.meta[b * 3 + 2];
    int* out = a.out + a.meta[b * 3 + 2];
    const unsigned long long* uni = a.uni + (long long)b * a.nw;
    const unsigned* prefix = a.prefix + (long long)b * a.nw;
    const unsigned* bs = a.bsum + (size_t)b * a.nsb;
    const unsigned total = a.n_other[b];
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long long)gridDim.x * TPB) {
        const int rank = ranks[i];
        if (rank < 0 || (unsigned)rank >= total) { out[i] = 0; continue; }
        const unsigned q = (unsigned)rank;
        int lo = 0, hi = a.nsb - 1;                        // the last scan block whose sum-before is <= q
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (bs[mid] <= q) lo = mid; else hi = mid - 1;
        }
        const unsigned r0 = q - bs[lo];
        long long k0 = (long long)lo * TPB, k1 = min(a.nw, k0 + TPB) - 1;      // the last word of it whose prefix is <= r0
        while (k0 < k1) {
            const long long mid = (k0 + k1 + 1) >> 1;
            if (prefix[mid] <= r0) k0 = mid; else k1 = mid - 1;
        }
        unsigned r = r0 - prefix[k0];
        unsigned long long x = uni[k0];
        int bit = 0;
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            const unsigned long long low = x & ((1ull << s) - 1ull);
            const unsigned c = (unsigned)__popcll(low);
            if (r >= c) { r -= c; x >>= s; bit += s; } else x = low;
        }
        out[i] = (int)(k0 * 64 + bit);
    }
}

}  // namespace

LaunchDesc p3d_fix_pack_desc(const FixPackArgs& a) {
    const double e = (double)a.n * (double)a.n_pix;
    return {"fix_pack_kernel", e, e + e / 8.0};
}

hipError_t p3d_fix_pack_launch(const FixPackArgs& a, hipStream_t s) {
    if (!a.maps || !a.words || ((uintptr_t)a.words & 7) || a.n < 1 || a.n > 65535 || a.n_pix < 1 || a.n_pix > (1ll << 30)) return hipErrorInvalidValue;
    const long long nw = p3d_fix_words(a.n_pix);
    const unsigned gx = (unsigned)std::min<long long>((nw + TPB / 64 - 1) / (TPB / 64), 2048);
    hipLaunchKernelGGL(fix_pack_kernel, dim3(gx, (unsigned)a.n), dim3(TPB), 0, s, a);
    return hipGetLastError();
}

LaunchDesc p3d_fix_union_desc(const FixUnionArgs& a) {
    const double e = (double)a.B * (double)a.nw;
    return {"fix_union_kernel", e * a.M, e * 8.0 * a.M + e * 12.0};
}

hipError_t p3d_fix_union_launch(const FixUnionArgs& a, hipStream_t s) {
    if (!a.pool || !a.ids || !a.uni || !a.prefix || !a.bsum || !a.n_other || !a.counter) return hipErrorInvalidValue;
    if (a.B < 1 || a.B > 65535 || a.M < 1 || a.M > 64 || a.nw < 1 || a.nw > (1ll << 24) || a.nsb != p3d_fix_scan_blocks(a.nw)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fix_union_kernel, dim3((unsigned)a.nsb, (unsigned)a.B), dim3(TPB), 0, s, a);
    return hipGetLastError();
}

LaunchDesc p3d_fix_select_desc(const FixSelectArgs& a) {
    const double e = (double)a.B * (double)a.max_rows * a.n_rep;
    return {"fix_select_kernel", e * 32.0, e * 24.0};
}

hipError_t p3d_fix_select_launch(const FixSelectArgs& a, hipStream_t s) {
    if (!a.uni || !a.prefix || !a.bsum || !a.n_other || !a.meta || !a.n_rows || !a.ranks || !a.out) return hipErrorInvalidValue;
    if (a.B < 1 || a.B > 65535 || a.n_rep < 1 || a.max_rows < 1 || a.nw < 1 || a.nsb != p3d_fix_scan_blocks(a.nw)) return hipErrorInvalidValue;
    const long long n = (long long)a.max_rows * a.n_rep;
    hipLaunchKernelGGL(fix_select_kernel, dim3((unsigned)std::min<long long>((n + TPB - 1) / TPB, 4096), (unsigned)a.B), dim3(TPB), 0, s, a);
    return hipGetLastError();
}
