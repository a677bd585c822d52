// Reframing around 8-bit saliency maps (p3d_video_reframe, p3d_reframe_u8; ReframeArgs in p3d_kernels.h, the law in
// include/p3d_hip.h, "Reframing around 8-bit maps"): per map the hc x wc window of the largest gated mass, a box-smoothed track of
// those windows over the call's n maps, the three masses of every map, and the windows cut out of the frames.  Integer arithmetic
// throughout: no order can show.
//
// The window sums come from a summed-area table per map, uint32 [H][W] in scratch (the largest entry is 255 * 2^23 < 2^31),
// p3d_reframe_plan's maps_per_chunk maps at a time; per chunk:
//  * reframe_rows: grid (ceil(H / 4), maps), one wave a row.  The row is read once in the 16-byte words of its own alignment, a
//    lane a word, 64 words a step; a word that holds bytes outside the row (the ragged head and tail) is read byte by byte and
//    only inside the row.  The gated bytes are summed in the lane, scanned over the wave by shuffles, carried from step to step;
//    the row's inclusive prefix sums go out as 16-byte words where the table's alignment allows.
//  * reframe_cols: grid (ceil(W / 64), maps), a lane a column, running sums down the rows, eight rows' loads in flight.
//  * reframe_search: grid (search_blocks, maps), a block takes positions_per_block window positions in row-major order (a lane
//    consecutive x0: the four table reads of a wave are contiguous), forms M from four corners and keeps the best under the tie
//    law -- M down, D up, position up; the position is unique, so the order is total and a reduction in any order gives the same
//    window.  Mass (31 bits), D (24) and position (23) do not fit one 64-bit key: the best is three words, compared in turn.
//    One best per block goes to scratch.
//  * reframe_pick: grid (maps), folds the blocks' bests of a map -- a launch of its own in place of an arrival counter: the fold
//    reads other blocks' stores, and the next launch sees them without any protocol -- and writes the raw track, M_best and T.
// Then, once over the n maps:
//  * reframe_track: a thread a frame, the box average of the raw track round frame f (64-bit sums, ends repeated); under a shot
//    table (ReframeArgs::starts) reframe_track_shots in its place: the ends of the frame's shot repeat.
//  * reframe_mass: grid (REFRAME_MASS_SLICES, n), M of the window at the smoothed position re-summed from the map's bytes (the
//    table of an earlier chunk is gone by now): a block a slice of the window's rows, a wave a row, in the same words as
//    reframe_rows; one sum per block to scratch, and reframe_mass_fold, a thread a frame, adds a frame's slices.  (One block a
//    frame took 0.67 ms for 64 windows of 1080 x 608, more than everything else together.)
//  * reframe_crop: grid (ceil(hc / 4), n), one wave a row of 3 wc bytes.  The destination decides the words: single bytes up to
//    its first 16-byte boundary, 16-byte stores, single bytes.  The source of a row starts at 3 (W (Y + y) + X) and almost never
//    agrees with the destination modulo 16, so a stored word is cut out of the two aligned source words it straddles (two
//    16-byte loads and a funnel shift by bytes; one load where the two agree).  Aligned words that reach outside the frames'
//    buffer are never loaded: such a word's 16 bytes are copied one by one.
#include "p3d_kernels.h"
#include "../../include/p3d_hip.h"
#include <algorithm>

namespace {

constexpr int TPB = 256, WAVE = 64, ROWS_PER_BLOCK = TPB / WAVE;
constexpr int COLS_TPB = 64;
constexpr int PER_THREAD = REFRAME_POSITIONS / TPB;
static_assert(PER_THREAD * TPB == REFRAME_POSITIONS, "a block's positions are whole rounds of its threads");

__device__ __forceinline__ unsigned dword_of(const uint4& v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }
__device__ __forceinline__ unsigned byte_of(const uint4& v, int j) { return (dword_of(v, j >> 2) >> ((j & 3) * 8)) & 255u; }
__device__ __forceinline__ unsigned weight(unsigned v, unsigned g) { return v >= g ? v : 0u; }

// The gated bytes of 16-byte word q of a run: the run's len bytes start off (0 .. 15) bytes into the aligned word at a0.  Bytes of
// the word outside the run are not read and weigh 0.
__device__ __forceinline__ void run_word(const unsigned char* a0, int off, int len, int q, unsigned g, unsigned w[16]) {
    const int x0 = q * 16 - off;
    if (x0 >= 0 && x0 + 16 <= len) {
        const uint4 v = *reinterpret_cast<const uint4*>(a0 + (size_t)q * 16);
#pragma unroll
        for (int j = 0; j < 16; ++j) w[j] = weight(byte_of(v, j), g);
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int x = x0 + j;
            w[j] = (x >= 0 && x < len) ? weight(a0[(size_t)q * 16 + j], g) : 0u;
        }
    }
}

__global__ __launch_bounds__(TPB) void reframe_rows(ReframeArgs a, int m0) {
    const int lane = threadIdx.x & (WAVE - 1), y = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6), m = blockIdx.y;
    if (y >= a.H) return;                                   // the whole wave: nothing below is shared between waves
    const unsigned char* ps = a.sal + ((size_t)(m0 + m) * a.H + y) * a.W;
    const int off = (int)((uintptr_t)ps & 15), words = (off + a.W + 15) >> 4;
    const unsigned char* a0 = ps - off;
    unsigned* row = a.sat + ((size_t)m * a.H + y) * a.W;
    const unsigned g = (unsigned)a.gate;
    unsigned carry = 0u;
    for (int q0 = 0; q0 < words; q0 += WAVE) {
        const int q = q0 + lane;
        unsigned w[16];
        if (q < words) {
            run_word(a0, off, a.W, q, g, w);
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) w[j] = 0u;
        }
#pragma unroll
        for (int j = 1; j < 16; ++j) w[j] += w[j - 1];
        const unsigned tot = w[15];
        unsigned inc = tot;
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            const unsigned t = __shfl_up(inc, d);
            if (lane >= d) inc += t;
        }
        const unsigned base = carry + inc - tot;
        const int x0 = q * 16 - off;
        if (q < words) {
            if (x0 >= 0 && x0 + 16 <= a.W && ((uintptr_t)(row + x0) & 15) == 0) {
                uint4* o = reinterpret_cast<uint4*>(row + x0);
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = make_uint4(base + w[4 * k], base + w[4 * k + 1], base + w[4 * k + 2], base + w[4 * k + 3]);
            } else {
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int x = x0 + j;
                    if (x >= 0 && x < a.W) row[x] = base + w[j];
                }
            }
        }
        carry += __shfl(inc, WAVE - 1);
    }
}

__global__ __launch_bounds__(COLS_TPB) void reframe_cols(ReframeArgs a) {
    const int x = blockIdx.x * COLS_TPB + threadIdx.x, m = blockIdx.y;
    if (x >= a.W) return;
    unsigned* p = a.sat + (size_t)m * a.H * a.W + x;
    const size_t W = (size_t)a.W;
    unsigned acc = 0u;
    int y = 0;
    for (; y + 8 <= a.H; y += 8) {
        unsigned v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = p[(size_t)(y + k) * W];
#pragma unroll
        for (int k = 0; k < 8; ++k) { acc += v[k]; p[(size_t)(y + k) * W] = acc; }
    }
    for (; y < a.H; ++y) { acc += p[(size_t)y * W]; p[(size_t)y * W] = acc; }
}

// A candidate window: its mass, its distance from the centred window, its position y0 * (W - wc + 1) + x0.  "No window" loses to all.
struct Best { unsigned M, D, p; };
__device__ __forceinline__ Best no_window() { return {0u, 0xffffffffu, 0xffffffffu}; }
__device__ __forceinline__ bool beats(const Best& c, const Best& b) {
    return c.M > b.M || (c.M == b.M && (c.D < b.D || (c.D == b.D && c.p < b.p)));
}
// The best of a block's candidates, in thread 0; slots: 3 * (TPB / WAVE) words of LDS
__device__ __forceinline__ Best block_best(Best b, unsigned* slots) {
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        const Best c = {(unsigned)__shfl_xor(b.M, o), (unsigned)__shfl_xor(b.D, o), (unsigned)__shfl_xor(b.p, o)};
        if (beats(c, b)) b = c;
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & (WAVE - 1)) == 0) { slots[3 * wave] = b.M; slots[3 * wave + 1] = b.D; slots[3 * wave + 2] = b.p; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 1; k < TPB / WAVE; ++k) {
            const Best c = {slots[3 * k], slots[3 * k + 1], slots[3 * k + 2]};
            if (beats(c, b)) b = c;
        }
    return b;
}

__global__ __launch_bounds__(TPB) void reframe_search(ReframeArgs a) {
    __shared__ unsigned slots[3 * (TPB / WAVE)];
    const int m = blockIdx.y, blk = blockIdx.x;
    const int Hp = a.H - a.hc + 1, Wp = a.W - a.wc + 1, P = Hp * Wp;
    const unsigned* S = a.sat + (size_t)m * a.H * a.W;
    Best b = no_window();
#pragma unroll 4
    for (int k = 0; k < PER_THREAD; ++k) {
        const int p = blk * REFRAME_POSITIONS + k * TPB + (int)threadIdx.x;
        if (p >= P) break;
        const int y0 = p / Wp, x0 = p - y0 * Wp, y1 = y0 + a.hc - 1, x1 = x0 + a.wc - 1;
        unsigned M = S[y1 * a.W + x1];
        if (y0 > 0) M -= S[(y0 - 1) * a.W + x1];
        if (x0 > 0) M -= S[y1 * a.W + x0 - 1];
        if (y0 > 0 && x0 > 0) M += S[(y0 - 1) * a.W + x0 - 1];
        const int dy = 2 * y0 - (Hp - 1), dx = 2 * x0 - (Wp - 1);
        const Best c = {M, (unsigned)((dy < 0 ? -dy : dy) + (dx < 0 ? -dx : dx)), (unsigned)p};
        if (beats(c, b)) b = c;
    }
    b = block_best(b, slots);
    if (threadIdx.x == 0) {
        unsigned* o = a.best + ((size_t)m * a.search_blocks + blk) * 3;
        o[0] = b.M; o[1] = b.D; o[2] = b.p;
    }
}

__global__ __launch_bounds__(TPB) void reframe_pick(ReframeArgs a, int m0) {
    __shared__ unsigned slots[3 * (TPB / WAVE)];
    const int m = blockIdx.x;
    const unsigned* in = a.best + (size_t)m * a.search_blocks * 3;
    Best b = no_window();
    for (int k = threadIdx.x; k < a.search_blocks; k += TPB) {
        const Best c = {in[3 * k], in[3 * k + 1], in[3 * k + 2]};
        if (beats(c, b)) b = c;
    }
    b = block_best(b, slots);
    if (threadIdx.x == 0) {
        const int Wp = a.W - a.wc + 1, f = m0 + m;
        a.raw[2 * f] = (int)(b.p / (unsigned)Wp);
        a.raw[2 * f + 1] = (int)(b.p % (unsigned)Wp);
        a.mass[3 * (size_t)f] = b.M;
        a.mass[3 * (size_t)f + 2] = a.sat[((size_t)m + 1) * a.H * a.W - 1];
    }
}

// a thread a frame: at most 511 taps of 64-bit adds
__global__ __launch_bounds__(TPB) void reframe_track(ReframeArgs a) {
    const int f = blockIdx.x * TPB + threadIdx.x;
    if (f >= a.n) return;
    const int R = a.radius;
    long long sy = 0, sx = 0;
    for (int k = -R; k <= R; ++k) {
        const int i = min(max(f + k, 0), a.n - 1);
        sy += a.raw[2 * i]; sx += a.raw[2 * i + 1];
    }
    const long long taps = 2 * R + 1;
    a.track[2 * f] = (int)((2 * sy + taps) / (2 * taps));
    a.track[2 * f + 1] = (int)((2 * sx + taps) / (2 * taps));
}

// The same average inside the frame's shot: starts [n_shots] ascending from 0, in frames of the call; the taps past an end of the
// shot repeat that end (c(i) = min(max(i, a), b)), so nothing of another shot enters and the window may jump at a cut.
__global__ __launch_bounds__(TPB) void reframe_track_shots(ReframeArgs a) {
    const int f = blockIdx.x * TPB + threadIdx.x;
    if (f >= a.n) return;
    int k = 0, top = a.n_shots - 1;                         // the last shot that starts at or before f
    while (k < top) {
        const int mid = (k + top + 1) >> 1;
        if (a.starts[mid] <= f) k = mid; else top = mid - 1;
    }
    const int lo = a.starts[k], hi = (k + 1 < a.n_shots ? a.starts[k + 1] : a.n) - 1;
    const int R = a.radius;
    long long sy = 0, sx = 0;
    for (int t = -R; t <= R; ++t) {
        const int i = min(max(f + t, lo), hi);
        sy += a.raw[2 * i]; sx += a.raw[2 * i + 1];
    }
    const long long taps = 2 * R + 1;
    a.track[2 * f] = (int)((2 * sy + taps) / (2 * taps));
    a.track[2 * f + 1] = (int)((2 * sx + taps) / (2 * taps));
}

// M at the smoothed position, from the bytes: block (s, f) sums slice s of the window's rows into part[f][s]
__global__ __launch_bounds__(TPB) void reframe_mass(ReframeArgs a) {
    __shared__ unsigned wsum[TPB / WAVE];
    const int s = blockIdx.x, f = blockIdx.y, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
    const int Y = a.track[2 * f], X = a.track[2 * f + 1];
    const int per = (a.hc + REFRAME_MASS_SLICES - 1) / REFRAME_MASS_SLICES, y_end = min(a.hc, (s + 1) * per);
    const unsigned char* ms = a.sal + (size_t)f * a.H * a.W;
    const unsigned g = (unsigned)a.gate;
    unsigned acc = 0u;
    for (int y = s * per + wave; y < y_end; y += TPB / WAVE) {
        const unsigned char* ps = ms + (size_t)(Y + y) * a.W + X;
        const int off = (int)((uintptr_t)ps & 15), words = (off + a.wc + 15) >> 4;
        for (int q = lane; q < words; q += WAVE) {
            unsigned w[16];
            run_word(ps - off, off, a.wc, q, g, w);
#pragma unroll
            for (int j = 0; j < 16; ++j) acc += w[j];
        }
    }
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) wsum[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        unsigned t = 0u;
        for (int k = 0; k < TPB / WAVE; ++k) t += wsum[k];
        a.part[(size_t)f * REFRAME_MASS_SLICES + s] = t;
    }
}

__global__ __launch_bounds__(TPB) void reframe_mass_fold(ReframeArgs a) {
    const int f = blockIdx.x * TPB + threadIdx.x;
    if (f >= a.n) return;
    unsigned t = 0u;
    for (int s = 0; s < REFRAME_MASS_SLICES; ++s) t += a.part[(size_t)f * REFRAME_MASS_SLICES + s];
    a.mass[3 * (size_t)f + 1] = t;
}

// bytes s .. s + 15 of the 32 bytes (A, B), s in 0 .. 15
__device__ __forceinline__ uint4 cut_word(const uint4& A, const uint4& B, int s) {
    const unsigned w[8] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w};
    const int d = s >> 2, sh = (s & 3) * 8;
    unsigned r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned lo = d == 0 ? w[k] : d == 1 ? w[k + 1] : d == 2 ? w[k + 2] : w[k + 3];
        const unsigned hi = d == 0 ? w[k + 1] : d == 1 ? w[k + 2] : d == 2 ? w[k + 3] : w[k + 4];
        r[k] = (unsigned)(((((unsigned long long)hi) << 32) | lo) >> sh);
    }
    return make_uint4(r[0], r[1], r[2], r[3]);
}

__global__ __launch_bounds__(TPB) void reframe_crop(ReframeArgs a) {
    const int lane = threadIdx.x & (WAVE - 1), y = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6), f = blockIdx.y;
    if (y >= a.hc) return;
    const int Y = a.track[2 * f], X = a.track[2 * f + 1];
    const unsigned char* lo = a.frames;
    const unsigned char* hi = a.frames + (size_t)a.n * a.H * a.W * 3;
    const unsigned char* src = a.frames + (((size_t)f * a.H + (size_t)(Y + y)) * a.W + X) * 3;
    unsigned char* dst = a.out + ((size_t)f * a.hc + y) * a.wc * 3;
    const int len = 3 * a.wc;
    const int head = min(len, (int)((16 - ((uintptr_t)dst & 15)) & 15)), words = (len - head) >> 4;
    const int s = (int)((uintptr_t)(src + head) & 15);
    const unsigned char* sa = src + head - s;               // aligned; the stored word q is bytes s .. s + 15 of the 32 at sa + 16 q
    for (int q = lane; q < words; q += WAVE) {
        const unsigned char* pa = sa + (size_t)q * 16;
        unsigned char* po = dst + head + (size_t)q * 16;
        if (pa >= lo && (s == 0 || pa + 32 <= hi)) {
            const uint4 A = *reinterpret_cast<const uint4*>(pa);
            const uint4 B = s ? *reinterpret_cast<const uint4*>(pa + 16) : A;
            *reinterpret_cast<uint4*>(po) = cut_word(A, B, s);
        } else {
            for (int j = 0; j < 16; ++j) po[j] = pa[s + j];
        }
    }
    const int body = words * 16, rest = len - body;
    for (int e = lane; e < rest; e += WAVE) {
        const int i = e < head ? e : e + body;
        dst[i] = src[i];
    }
}

bool args_ok(const ReframeArgs& a) {
    if (!a.sal || !a.track || !a.raw || !a.mass || !a.sat || !a.best || !a.part) return false;
    if ((a.frames == nullptr) != (a.out == nullptr)) return false;
    if ((a.starts == nullptr) != (a.n_shots == 0) || a.n_shots < 0 || a.n_shots > a.n) return false;
    if (a.n < 1 || a.n > 65535 || a.H < 1 || a.W < 1 || (long long)a.H * a.W > P3D_REFRAME_MAX_PIXELS) return false;
    if (a.hc < 1 || a.hc > a.H || a.wc < 1 || a.wc > a.W || a.gate < 0 || a.gate > 255 || a.radius < 0 || a.radius > 255) return false;
    const ReframePlan p = p3d_reframe_plan(a.H, a.W, a.hc, a.wc, a.n);
    return a.maps_per_chunk == p.maps_per_chunk && a.search_blocks == p.search_blocks;
}

}  // namespace

ReframePlan p3d_reframe_plan(int H, int W, int hc, int wc, int n) {
    ReframePlan p;
    const long long hw = (long long)H * W, positions = (long long)(H - hc + 1) * (W - wc + 1);
    p.maps_per_chunk = (int)std::max<long long>(1, std::min<long long>(std::min(n, P3D_REFRAME_CHUNK), P3D_REFRAME_SAT_BYTES / (4 * hw)));
    p.positions_per_block = REFRAME_POSITIONS;
    p.search_blocks = (int)((positions + REFRAME_POSITIONS - 1) / REFRAME_POSITIONS);
    p.sat_elems = (long long)p.maps_per_chunk * hw;
    p.best_elems = (long long)p.maps_per_chunk * p.search_blocks * 3;
    p.part_elems = (long long)n * REFRAME_MASS_SLICES;
    // three buffers, each from a 256-byte boundary
    p.scratch_bytes = ((p.sat_elems * 4 + 255) & ~255LL) + ((p.best_elems * 4 + 255) & ~255LL) + ((p.part_elems * 4 + 255) & ~255LL);
    return p;
}

hipError_t p3d_reframe_launch(const ReframeArgs& a, hipStream_t s) {
    if (!args_ok(a)) return hipErrorInvalidValue;
    const dim3 block(TPB);
    for (int m0 = 0; m0 < a.n; m0 += a.maps_per_chunk) {
        const unsigned maps = (unsigned)std::min(a.maps_per_chunk, a.n - m0);
        hipLaunchKernelGGL(reframe_rows, dim3((unsigned)((a.H + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK), maps), block, 0, s, a, m0);
        hipLaunchKernelGGL(reframe_cols, dim3((unsigned)((a.W + COLS_TPB - 1) / COLS_TPB), maps), dim3(COLS_TPB), 0, s, a);
        hipLaunchKernelGGL(reframe_search, dim3((unsigned)a.search_blocks, maps), block, 0, s, a);
        hipLaunchKernelGGL(reframe_pick, dim3(maps), block, 0, s, a, m0);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const dim3 frames((unsigned)((a.n + TPB - 1) / TPB));
    if (a.starts) hipLaunchKernelGGL(reframe_track_shots, frames, block, 0, s, a);
    else hipLaunchKernelGGL(reframe_track, frames, block, 0, s, a);
    hipLaunchKernelGGL(reframe_mass, dim3(REFRAME_MASS_SLICES, (unsigned)a.n), block, 0, s, a);
    hipLaunchKernelGGL(reframe_mass_fold, frames, block, 0, s, a);
    if (a.frames) hipLaunchKernelGGL(reframe_crop, dim3((unsigned)((a.hc + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK), (unsigned)a.n), block, 0, s, a);
    return hipGetLastError();
}
