// Block importance and QP offsets of 8-bit saliency maps (p3d_video_qpmap, p3d_qpmap_u8; QpmapArgs in p3d_kernels.h, the law in
// include/p3d_hip.h, "QP maps of 8-bit maps"): per map the level of every coding block, dilated, turned into a quantiser offset by a
// table, limited from frame to frame inside the shots, and balanced per frame.  Integer arithmetic throughout and no atomics: every
// sum is an integer sum folded in LDS, so no order can show.
//
// Each step is a launch of its own -- a launch boundary is the fence that makes one step's stores visible to the next:
//  * qpmap_reduce (the hot path; p3d_qpmap_plan's maps_per_chunk maps at a time): grid (tiles_x * Hb, maps), a block a STRIP of `block`
//    rows, QPMAP_TILE_WORDS * 16 columns wide.  A thread owns one 16-byte CHUNK of columns (16 q .. 16 q + 15 of the row, so a chunk
//    lies in one coding block, or in two at block = 8) and every G-th row of the strip, G = the threads left over by the chunks of a
//    row: SUM and MAX of the chunk's two halves stay in registers over the rows.  A chunk comes in as the one or two ALIGNED 16-byte
//    words that hold it (two when the row's address is not a multiple of 16; the neighbour lane reads the same word, so HBM gives
//    every byte once) and a funnel shift by the row's phase; a word that reaches outside [sal, sal + n H W) is read byte by byte,
//    inside only.  The registers are then folded in LDS across the row groups and across the chunks that share a coding block, and
//    one thread a block writes its level.
//  * qpmap_law: a thread a block of the grid; the largest level of the (2 dilate + 1)^2 neighbourhood, and the law's entry.
//  * qpmap_limit (fall or rise set): a lane a block position walks the frames of the call in order, as temporal.hip's moving
//    average does, and restarts at every shot start.  The loads of LIMIT_FRAMES frames go out together, so that the walk waits
//    for memory once per that many frames, and a frame the limiter leaves alone is not written.
//  * qpmap_balance: a block a frame; S1, the shift, the clamp and the statistics.
#include "p3d_kernels.h"
#include "../../include/p3d_hip.h"
#include <algorithm>
#include <climits>

namespace {

constexpr int TPB = 256, WAVE = 64, TILE_WORDS = QPMAP_TILE_WORDS;
constexpr int LIMIT_FRAMES = 16;                         // frames of the limiter whose loads are in flight together

__device__ __forceinline__ unsigned sum4(unsigned x) { return __builtin_amdgcn_sad_u8(x, 0u, 0u); }
__device__ __forceinline__ unsigned max4(unsigned x) { return max(max(x & 255u, (x >> 8) & 255u), max((x >> 16) & 255u, x >> 24)); }

// The aligned 16-byte word at address w; its bytes outside [base, end) read as 0 and are not touched
__device__ __forceinline__ uint4 word_at(uintptr_t w, uintptr_t base, uintptr_t end) {
    if (w >= base && w + 16 <= end) return *reinterpret_cast<const uint4*>(w);
    unsigned d[4] = {0u, 0u, 0u, 0u};
    for (int j = 0; j < 16; ++j) {
        const uintptr_t at = w + (uintptr_t)j;
        if (at >= base && at < end) d[j >> 2] |= (unsigned)*reinterpret_cast<const unsigned char*>(at) << ((j & 3) * 8);
    }
    return make_uint4(d[0], d[1], d[2], d[3]);
}

// The 16 bytes from address p on, which lies in [base, end); bytes from `valid` (1 .. 16) on are 0 and are never fetched word-wise
// unless their word holds wanted bytes too
__device__ __forceinline__ uint4 load_chunk(uintptr_t p, uintptr_t base, uintptr_t end, int valid) {
    const unsigned phase = (unsigned)(p & 15);
    const uintptr_t w0 = p - phase;
    const uint4 lo = word_at(w0, base, end);
    uint4 hi = make_uint4(0u, 0u, 0u, 0u);
    if (phase + (unsigned)valid > 16u) hi = word_at(w0 + 16, base, end);
    // whole dwords first (k), then bits
    const unsigned k = phase >> 2, bits = (phase & 3u) * 8u;
    const unsigned d[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    unsigned t[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) t[j] = k == 0 ? d[j] : k == 1 ? d[j + 1] : k == 2 ? d[j + 2] : d[j + 3];
    unsigned o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        o[j] = __funnelshift_r(t[j], t[j + 1], bits);       // bits = 0: t[j]
        const int keep = valid - 4 * j;                    // bytes of this dword inside the row
        o[j] = keep >= 4 ? o[j] : keep <= 0 ? 0u : o[j] & ((1u << (8 * keep)) - 1u);
    }
    return make_uint4(o[0], o[1], o[2], o[3]);
}

__device__ __forceinline__ int log2_of(int block) { return __ffs(block) - 1; }

__global__ __launch_bounds__(TPB) void qpmap_reduce(QpmapArgs a, int m0) {
    __shared__ unsigned ps[2][TPB], pm[2][TPB];
    const int tid = threadIdx.x;
    const int tile = (int)(blockIdx.x % (unsigned)a.tiles_x), by = (int)(blockIdx.x / (unsigned)a.tiles_x), m = m0 + (int)blockIdx.y;
    const int B = a.block, sh = log2_of(B);
    const int c0 = tile * TILE_WORDS;                       // the tile's first chunk of the row
    const int cw = min(TILE_WORDS, ((a.W + 15) >> 4) - c0);  // its chunks, 1 .. TILE_WORDS
    const int G = TPB / cw;                                 // rows in flight
    const int q = tid % cw, g = tid / cw;
    const int y0 = by * B, rows = min(B, a.H - y0);
    unsigned s0 = 0u, s1 = 0u, x0 = 0u, x1 = 0u;            // SUM and MAX of the chunk's low and high 8 bytes over this thread's rows
    if (g < G) {
        const uintptr_t base = (uintptr_t)a.sal, end = base + (size_t)a.n * (size_t)a.H * (size_t)a.W;
        const int col = (c0 + q) << 4, valid = min(16, a.W - col);
#pragma unroll 4
        for (int r = g; r < rows; r += G) {
            const uintptr_t p = base + ((size_t)m * (size_t)a.H + (size_t)(y0 + r)) * (size_t)a.W + (size_t)col;
            const uint4 v = load_chunk(p, base, end, valid);
            s0 += sum4(v.x) + sum4(v.y); s1 += sum4(v.z) + sum4(v.w);
            x0 = max(x0, max(max4(v.x), max4(v.y))); x1 = max(x1, max(max4(v.z), max4(v.w)));
        }
    }
    ps[0][tid] = s0; ps[1][tid] = s1; pm[0][tid] = x0; pm[1][tid] = x1;   // (threads with g >= G: zeroes nobody reads)
    __syncthreads();
    // the coding blocks of this tile: two a chunk at B = 8, else one per B / 16 chunks (a tile starts on a block's edge)
    const int bx0 = (c0 << 4) >> sh;
    const int nb = min(a.Wb - bx0, B == 8 ? 2 * cw : (cw * 16 + B - 1) >> sh);
    const int cpb = B == 8 ? 1 : B >> 4;
    for (int j = tid; j < nb; j += TPB) {
        const int qa = B == 8 ? j >> 1 : j * cpb, qb = min(cw, qa + cpb);
        unsigned sum = 0u, mx = 0u;
        for (int gg = 0; gg < G; ++gg)
            for (int qq = qa; qq < qb; ++qq) {
                const int t = gg * cw + qq;
                if (B == 8) { sum += ps[j & 1][t]; mx = max(mx, pm[j & 1][t]); }
                else { sum += ps[0][t] + ps[1][t]; mx = max(mx, max(pm[0][t], pm[1][t])); }
            }
        const int bx = bx0 + j;
        const unsigned area = (unsigned)rows * (unsigned)(min(a.W, (bx + 1) << sh) - (bx << sh));
        const unsigned mean = (2u * sum + area) / (2u * area);
        const unsigned level = ((unsigned)a.peak_weight * mx + (unsigned)(256 - a.peak_weight) * mean + 128u) >> 8;
        a.lev0[((size_t)blockIdx.y * (size_t)a.Hb + (size_t)by) * (size_t)a.Wb + (size_t)bx] = (unsigned char)level;
    }
}

__global__ __launch_bounds__(TPB) void qpmap_law(QpmapArgs a, int m0, int maps) {
    const long long cells = (long long)a.Hb * a.Wb, i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= cells * maps) return;
    const int mm = (int)(i / cells), at = (int)(i - (long long)mm * cells), by = at / a.Wb, bx = at - by * a.Wb;
    const unsigned char* lev = a.lev0 + (size_t)mm * (size_t)cells;
    const int ya = max(0, by - a.dilate), yb = min(a.Hb - 1, by + a.dilate), xa = max(0, bx - a.dilate), xb = min(a.Wb - 1, bx + a.dilate);
    unsigned level = 0u;
    for (int y = ya; y <= yb; ++y)
        for (int x = xa; x <= xb; ++x) level = max(level, (unsigned)lev[(size_t)y * a.Wb + x]);
    const size_t out = (size_t)(m0 + mm) * (size_t)cells + (size_t)at;
    if (a.levels) a.levels[out] = (unsigned char)level;
    a.qp[out] = a.law[level];
}

__global__ __launch_bounds__(TPB) void qpmap_limit(QpmapArgs a) {
    const long long cells = (long long)a.Hb * a.Wb, i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= cells) return;
    int32_t* const col = a.qp + (size_t)i;                  // this block position, frame f at f * cells
    int si = 0, next = a.starts ? a.starts[0] : INT_MAX, prev = 0;      // next: the first start of the table not yet behind the walk
    for (int f0 = 0; f0 < a.n; f0 += LIMIT_FRAMES) {
        // the loads of LIMIT_FRAMES frames go out together: only the recurrence below is serial, not the trips to memory
        int q0[LIMIT_FRAMES];
#pragma unroll
        for (int j = 0; j < LIMIT_FRAMES; ++j) q0[j] = f0 + j < a.n ? col[(size_t)(f0 + j) * (size_t)cells] : 0;
#pragma unroll
        for (int j = 0; j < LIMIT_FRAMES; ++j) {
            const int f = f0 + j;
            if (f >= a.n) break;
            while (next < f) { ++si; next = si < a.n_shots ? a.starts[si] : INT_MAX; }      // ends: si only grows
            int q = q0[j];
            if (f != 0 && f != next) {
                if (a.fall) q = max(q, prev - a.fall);
                if (a.rise) q = min(q, prev + a.rise);
                if (q != q0[j]) col[(size_t)f * (size_t)cells] = q;
            }
            prev = q;
        }
    }
}

// the block's sum (largest) of v in every thread; red: a word of LDS a wave
__device__ __forceinline__ int block_sum(int v, int* red) {
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();                                         // (red may still be read from the call before)
    if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = v;
    __syncthreads();
    int sum = 0;
#pragma unroll
    for (int w = 0; w < TPB / WAVE; ++w) sum += red[w];
    return sum;
}
__device__ __forceinline__ int block_max(int v, int* red) {
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    __syncthreads();
    if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = v;
    __syncthreads();
    int top = red[0];
#pragma unroll
    for (int w = 1; w < TPB / WAVE; ++w) top = max(top, red[w]);
    return top;
}

__global__ __launch_bounds__(TPB) void qpmap_balance(QpmapArgs a) {
    __shared__ int red[TPB / WAVE];
    const int f = (int)blockIdx.x, cells = a.Hb * a.Wb, sh = log2_of(a.block);
    int32_t* const q = a.qp + (size_t)f * (size_t)cells;
    int part = 0;
    for (int i = threadIdx.x; i < cells; i += TPB) {
        const int by = i / a.Wb, bx = i - by * a.Wb;
        const int area = (min(a.H, (by + 1) << sh) - (by << sh)) * (min(a.W, (bx + 1) << sh) - (bx << sh));
        part += area * q[i];
    }
    const int S1 = block_sum(part, red);
    int shift = 0;
    if (a.balance) {
        const long long A = (long long)a.H * a.W, num = 2LL * S1 + A, den = 2LL * A;
        long long mean = num / den;
        if (num % den != 0 && num < 0) --mean;               // towards minus infinity
        shift = a.target - (int)mean;
    }
    int lo = INT_MAX, hi = INT_MIN, part2 = 0;
    for (int i = threadIdx.x; i < cells; i += TPB) {
        const int by = i / a.Wb, bx = i - by * a.Wb;
        const int area = (min(a.H, (by + 1) << sh) - (by << sh)) * (min(a.W, (bx + 1) << sh) - (bx << sh));
        const int q2 = min(max(q[i] + shift, a.lo), a.hi);
        q[i] = q2;
        lo = min(lo, q2); hi = max(hi, q2); part2 += area * q2;
    }
    if (!a.stats) return;                                    // (uniform: nobody waits below)
    const int S2 = block_sum(part2, red), top = block_max(hi, red), bottom = -block_max(-lo, red);
    if (threadIdx.x == 0) {
        int32_t* const st = a.stats + (size_t)f * 4;
        st[0] = bottom; st[1] = top; st[2] = S1; st[3] = S2;
    }
}

bool block_ok(int B) { return B == 8 || B == 16 || B == 32 || B == 64 || B == 128; }

bool args_ok(const QpmapArgs& a) {
    if (!a.sal || !a.law || !a.qp || !a.lev0) return false;
    if (a.n < 1 || a.n > 65535 || a.H < 1 || a.W < 1 || (long long)a.H * a.W > P3D_QPMAP_MAX_PIXELS) return false;
    if (!block_ok(a.block) || a.peak_weight < 0 || a.peak_weight > 256 || a.dilate < 0 || a.dilate > 8) return false;
    if (a.fall < 0 || a.fall > 254 || a.rise < 0 || a.rise > 254 || (a.balance != 0 && a.balance != 1)) return false;
    if (a.lo < -127 || a.lo > a.target || a.target > a.hi || a.hi > 127) return false;
    if ((a.starts == nullptr) != (a.n_shots == 0) || a.n_shots < 0 || a.n_shots > a.n) return false;
    const QpmapPlan p = p3d_qpmap_plan(a.H, a.W, a.block, a.n);
    return a.maps_per_chunk == p.maps_per_chunk && a.Hb == p.Hb && a.Wb == p.Wb && a.tiles_x == p.tiles_x;
}

}  // namespace

QpmapPlan p3d_qpmap_plan(int H, int W, int block, int n) {
    QpmapPlan p;
    if (!block_ok(block)) return p;
    p.Hb = (H + block - 1) / block; p.Wb = (W + block - 1) / block;
    const int words = (W + 15) / 16;
    p.strip_rows = block; p.tile_cols = std::min(W, TILE_WORDS * 16);
    p.tiles_x = (words + TILE_WORDS - 1) / TILE_WORDS;
    p.blocks_per_map = p.tiles_x * p.Hb;
    p.maps_per_chunk = std::max(1, std::min(n, P3D_QPMAP_CHUNK));
    p.lev0_elems = (long long)p.maps_per_chunk * p.Hb * p.Wb;
    p.scratch_bytes = (p.lev0_elems + 255) & ~255LL;        // from a 256-byte boundary
    return p;
}

hipError_t p3d_qpmap_launch(const QpmapArgs& a, hipStream_t s) {
    if (!args_ok(a)) return hipErrorInvalidValue;
    const long long cells = (long long)a.Hb * a.Wb;
    for (int m0 = 0; m0 < a.n; m0 += a.maps_per_chunk) {
        const int maps = std::min(a.maps_per_chunk, a.n - m0);
        hipLaunchKernelGGL(qpmap_reduce, dim3((unsigned)(a.tiles_x * a.Hb), (unsigned)maps), dim3(TPB), 0, s, a, m0);
        hipLaunchKernelGGL(qpmap_law, dim3((unsigned)((cells * maps + TPB - 1) / TPB)), dim3(TPB), 0, s, a, m0, maps);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (a.fall || a.rise) hipLaunchKernelGGL(qpmap_limit, dim3((unsigned)((cells + TPB - 1) / TPB)), dim3(TPB), 0, s, a);
    hipLaunchKernelGGL(qpmap_balance, dim3((unsigned)a.n), dim3(TPB), 0, s, a);
    return hipGetLastError();
}
