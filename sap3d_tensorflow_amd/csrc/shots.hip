// Shot boundaries of 8-bit frames (p3d_shot_distances_u8, p3d_shot_cuts; ShotsArgs and ShotCutArgs in p3d_kernels.h, the law in
// include/p3d_hip.h, "Shot boundaries of 8-bit frames"): per frame a gy x gx grid of cells, per cell and channel a 64-bin histogram
// of byte >> 2; D_f is the sum of |h_f - h_{f-1}| over every cell, channel and bin; a cut is a D_f that is large against the frame
// and a peak against its neighbours.  Integer arithmetic throughout: no order can show.
//
//  * shots_count: grid (blocks_per_frame, frames of the chunk).  A block takes rows_per_block rows that lie inside ONE row of cells,
//    a wave a row at a time.  The row's 3 W bytes are read in the 16-byte words of its own alignment, a lane a word, 64 words a step,
//    between a head and a tail of single bytes (at most 15 each, one lane a byte).  Byte i of a row belongs to pixel i / 3 and
//    channel i mod 3 -- of its position in the ROW, not of its address: a word that starts at byte i0 has x0 = i0 / 3 and the phase
//    i0 - 3 x0, and byte j of it is pixel x0 + (phase + j) / 3, channel (phase + j) mod 3.  The column of cells of pixel x is the
//    number of the boundaries ceil(c W / gx), c = 1 .. gx - 1, at or below x (x gx / W >= c exactly when x >= ceil(c W / gx)).
//    Every wave counts into a table [gx][192] of its own in LDS; the block's four are added up and the non-zero sums flushed with
//    integer atomics to the frame's table [gy][gx][3][64] (zeroed by the launcher in stream order).
//    BALLOT: the bin of every lane goes through score_u8.hip's count_bin (equal bins of a wave retire with one add of their number)
//    instead of one LDS add a byte.  Same counts; which is faster is in DESIGN.md.
//  * shots_dist: a block a frame of the chunk, |h_f - h_{f-1}| summed over the table's words in 32 bits (the total is at most
//    6 H W <= 6 * 2^28 < 2^32) -- a launch of its own in place of an arrival counter: it reads what the count's atomics wrote, and
//    the next launch sees them without any protocol.  Slot 0 of the tables is the chunk before's last frame.
//  * shots_cuts: one block.  Every thread decides CAND of its frames (at most 2 * 32 neighbours each) into scratch; thread 0 then
//    walks the frames in order and applies ACCEPT.
#include "p3d_kernels.h"
#include "../../include/p3d_hip.h"
#include <algorithm>

namespace {

constexpr int TPB = 256, WAVE = 64, WAVES = TPB / WAVE;
constexpr int CELL_WORDS = 192;                            // three channels of 64 bins
constexpr int MIN_BLOCK_BYTES = 8 << 10, TARGET_BLOCKS = 2048;
constexpr int MAX_GRID = P3D_SHOTS_MAX_GRID;
static_assert(MAX_GRID == 4, "a column of cells is found from three boundaries");

struct CountArgs {
    const unsigned char* frames; unsigned* tabs;
    int H, W, gy, gx, rows_per_block;
    int by[MAX_GRID + 1];                                  // rows of cells: row r is image rows by[r] .. by[r + 1] - 1
    int nb[MAX_GRID + 1];                                  // blocks before row r of cells
    int bx[MAX_GRID - 1];                                  // first pixel of columns 1 .. 3 of cells (INT_MAX past gx - 1)
};

__device__ __forceinline__ unsigned dword_of(const uint4& v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }
__device__ __forceinline__ unsigned byte_of(const uint4& v, int j) { return (dword_of(v, j >> 2) >> ((j & 3) * 8)) & 255u; }

// one wave counts bin b of every lane (b < 0: the lane has none) into its table; every lane of the wave calls it
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

// the word of a wave's table that byte v at position i of its row counts into
__device__ __forceinline__ int bin_of(const CountArgs& a, int x, int ch, unsigned v) {
    const int cx = (x >= a.bx[0]) + (x >= a.bx[1]) + (x >= a.bx[2]);
    return cx * CELL_WORDS + ch * 64 + (int)(v >> 2);
}

template <bool BALLOT>
__device__ __forceinline__ void count_one(unsigned* cnt, int b, int lane) {
    if (BALLOT) count_bin(cnt, b, lane);
    else if (b >= 0) atomicAdd(&cnt[b], 1u);
}

// one row of len = 3 W bytes at p, by one wave, into the wave's table
template <bool BALLOT>
__device__ __forceinline__ void count_row(const CountArgs& a, unsigned* cnt, const unsigned char* p, int len, int lane) {
    const int head = min(len, (int)((16 - ((uintptr_t)p & 15)) & 15)), words = (len - head) >> 4;
    for (int q0 = 0; q0 < words; q0 += WAVE) {             // a wave-uniform trip count: the ballots need every lane
        const int q = q0 + lane;
        const bool on = q < words;
        const int i0 = head + q * 16, x0 = i0 / 3, phase = i0 - 3 * x0;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (on) v = *reinterpret_cast<const uint4*>(p + i0);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int t = phase + j, dx = t / 3;           // t <= 17
            count_one<BALLOT>(cnt, on ? bin_of(a, x0 + dx, t - 3 * dx, byte_of(v, j)) : -1, lane);
        }
    }
    // the head and the tail: at most 15 + 15 single bytes, a lane a byte
    const int body = words * 16, rest = len - body;
    int b = -1;
    if (lane < rest) {
        const int i = lane < head ? lane : lane + body, x = i / 3;
        b = bin_of(a, x, i - 3 * x, p[i]);
    }
    count_one<BALLOT>(cnt, b, lane);
}

// the frame's table gets what the block's waves counted; cnt: the cell row's part of it
__device__ __forceinline__ void flush(unsigned* cnt, const unsigned* lds, int words, int tid) {
    for (int t = tid; t < words; t += TPB) {
        unsigned s = 0u;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) s += lds[w * MAX_GRID * CELL_WORDS + t];
        if (s) atomicAdd(&cnt[t], s);
    }
}

template <bool BALLOT>
__global__ __launch_bounds__(TPB) void shots_count(CountArgs a, int f0) {
    __shared__ unsigned lds[WAVES * MAX_GRID * CELL_WORDS];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6, c = blockIdx.y;
    for (int t = tid; t < WAVES * MAX_GRID * CELL_WORDS; t += TPB) lds[t] = 0u;
    __syncthreads();
    int cy = 0;
    while (cy + 1 < a.gy && (int)blockIdx.x >= a.nb[cy + 1]) ++cy;
    const int y0 = a.by[cy] + ((int)blockIdx.x - a.nb[cy]) * a.rows_per_block, y1 = min(a.by[cy + 1], y0 + a.rows_per_block);
    const int len = 3 * a.W;
    const unsigned char* frame = a.frames + (size_t)(f0 + c) * a.H * (size_t)len;
    unsigned* mine = lds + wave * MAX_GRID * CELL_WORDS;
    for (int y = y0 + wave; y < y1; y += WAVES) count_row<BALLOT>(a, mine, frame + (size_t)y * len, len, lane);
    __syncthreads();
    const int cell_row = a.gx * CELL_WORDS;
    flush(a.tabs + (size_t)(c + 1) * a.gy * cell_row + (size_t)cy * cell_row, lds, cell_row, tid);
}

__global__ __launch_bounds__(TPB) void shots_dist(const unsigned* tabs, int words, uint32_t* D, int f0) {
    __shared__ unsigned wsum[WAVES];
    const int tid = threadIdx.x, c = blockIdx.x;
    const unsigned* prev = tabs + (size_t)c * words;
    const unsigned* cur = prev + words;
    unsigned acc = 0u;
    if (f0 + c > 0)
        for (int t = tid; t < words; t += TPB) {
            const unsigned p = prev[t], q = cur[t];
            acc += p > q ? p - q : q - p;
        }
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((tid & (WAVE - 1)) == 0) wsum[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        unsigned t = 0u;
        for (int k = 0; k < WAVES; ++k) t += wsum[k];
        D[f0 + c] = t;
    }
}

__global__ __launch_bounds__(TPB) void shots_cuts(ShotCutArgs a) {
    const int tid = threadIdx.x;
    const unsigned long long floor_lhs = (unsigned long long)a.threshold_permille * 6ull * (unsigned long long)a.P;
    for (int f = tid; f < a.F; f += TPB) {
        unsigned is = 0u;
        if (f >= 1) {
            const unsigned long long d = a.D[f];
            unsigned nmax = 0u;
            for (int g = max(1, f - a.window); g <= min(a.F - 1, f + a.window); ++g)
                if (g != f) nmax = max(nmax, a.D[g]);
            is = d * 1000ull >= floor_lhs && d * 256ull >= (unsigned long long)a.ratio_q8 * nmax;
        }
        a.cand[f] = is;
    }
    __syncthreads();                                        // one block: its own stores to cand are visible behind the barrier
    if (tid == 0) {
        int last = 0, count = 1;
        if (a.cap > 0) a.starts[0] = 0;
        for (int f = 1; f < a.F; ++f)
            if (a.cand[f] && f - last >= a.min_length && a.F - f >= a.min_length) {
                if (count < a.cap) a.starts[count] = f;
                ++count;
                last = f;
            }
        *a.n_shots = count;
    }
}

int ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }

bool shape_ok(int n, int H, int W, int gy, int gx) {
    return n >= 1 && n <= 65535 && H >= 1 && W >= 1 && (long long)H * W <= P3D_SHOTS_MAX_PIXELS && gy >= 1 && gy <= std::min(MAX_GRID, H) &&
           gx >= 1 && gx <= std::min(MAX_GRID, W);
}

}  // namespace

ShotsPlan p3d_shots_plan(int H, int W, int gy, int gx, int n) {
    ShotsPlan p;
    p.frames_per_chunk = std::min(n, P3D_SHOTS_CHUNK);
    // rows that make about TARGET_BLOCKS blocks a launch, but whole rows of at least MIN_BLOCK_BYTES (a block zeroes and flushes its
    // tables whatever it counts) and at most SHOTS_BLOCK_BYTES, and a row a wave
    const int least = ceil_div(MIN_BLOCK_BYTES, 3LL * W), most = std::max(least, ceil_div(SHOTS_BLOCK_BYTES, 3LL * W));
    p.rows_per_block = std::max(WAVES, std::min(most, std::max(least, ceil_div((long long)H * p.frames_per_chunk, TARGET_BLOCKS))));
    for (int r = 0; r < gy; ++r) p.blocks_per_frame += ceil_div(ceil_div((long long)(r + 1) * H, gy) - ceil_div((long long)r * H, gy), p.rows_per_block);
    p.table_words = gy * gx * CELL_WORDS;
    p.scratch_bytes = (long long)(p.frames_per_chunk + 1) * p.table_words * 4;
    return p;
}

hipError_t p3d_shots_launch(const ShotsArgs& a, hipStream_t s) {
    if (!a.frames || !a.D || !a.tabs || !shape_ok(a.n, a.H, a.W, a.gy, a.gx)) return hipErrorInvalidValue;
    const ShotsPlan p = p3d_shots_plan(a.H, a.W, a.gy, a.gx, a.n);
    if (a.rows_per_block != p.rows_per_block || a.blocks_per_frame != p.blocks_per_frame || a.frames_per_chunk != p.frames_per_chunk)
        return hipErrorInvalidValue;
    CountArgs c;
    c.frames = a.frames; c.tabs = a.tabs; c.H = a.H; c.W = a.W; c.gy = a.gy; c.gx = a.gx; c.rows_per_block = p.rows_per_block;
    for (int r = 0; r <= MAX_GRID; ++r) { c.by[r] = a.H; c.nb[r] = p.blocks_per_frame; }
    int blocks = 0;
    for (int r = 0; r < a.gy; ++r) {
        c.by[r] = ceil_div((long long)r * a.H, a.gy);
        c.nb[r] = blocks;
        blocks += ceil_div(ceil_div((long long)(r + 1) * a.H, a.gy) - c.by[r], p.rows_per_block);
    }
    for (int k = 1; k < MAX_GRID; ++k) c.bx[k - 1] = k < a.gx ? ceil_div((long long)k * a.W, a.gx) : INT32_MAX;
    const size_t T = (size_t)p.table_words;
    for (int f0 = 0; f0 < a.n; f0 += p.frames_per_chunk) {
        const int m = std::min(p.frames_per_chunk, a.n - f0);
        hipError_t e = hipMemsetAsync(a.tabs + T, 0, (size_t)m * T * sizeof(unsigned), s);
        if (e != hipSuccess) return e;
        const dim3 grid((unsigned)p.blocks_per_frame, (unsigned)m);
        if (a.ballot) hipLaunchKernelGGL(shots_count<true>, grid, dim3(TPB), 0, s, c, f0);
        else hipLaunchKernelGGL(shots_count<false>, grid, dim3(TPB), 0, s, c, f0);
        hipLaunchKernelGGL(shots_dist, dim3((unsigned)m), dim3(TPB), 0, s, (const unsigned*)a.tabs, p.table_words, a.D, f0);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (f0 + m < a.n) {                                 // the last table seeds the next chunk
            e = hipMemcpyAsync(a.tabs, a.tabs + (size_t)m * T, T * sizeof(unsigned), hipMemcpyDeviceToDevice, s);
            if (e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

hipError_t p3d_shot_cuts_launch(const ShotCutArgs& a, hipStream_t s) {
    if (!a.D || !a.cand || !a.n_shots || a.F < 1 || a.F > 65535 || a.P < 1 || a.P > P3D_SHOTS_MAX_PIXELS || a.cap < 0 || (a.cap > 0 && !a.starts))
        return hipErrorInvalidValue;
    if (a.threshold_permille < 1 || a.threshold_permille > 1000 || a.window < 0 || a.window > 32 || a.ratio_q8 < 256 || a.ratio_q8 > 65535 ||
        a.min_length < 1)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(shots_cuts, dim3(1), dim3(TPB), 0, s, a);
    return hipGetLastError();
}

// ---- gradual transitions (p3d_shot_signals_u8, p3d_shot_transitions; the law in include/p3d_hip.h, "Gradual transitions") ----
//  * shots_signals: a block a frame of the chunk, behind shots_count.  Thread j < 192 is channel j / 64 (its wave) and bin j mod 64
//    (its lane): it walks the cells and reads word j of each cell of the frame's table, of the table before and of the table `lag`
//    frames back once -- |h_f - h_{f-1}| and |h_f - h_{f-lag}| in 32 bits, the bin's count over all cells n_b beside them.  S1 and S2
//    of a channel are then sums over the lanes of its wave, and lane 0 forms w_c with the header's q, r split: nothing above 64 bits.
//  * shots_transitions: one block.  Every thread decides CAND, MONO and HIGH of its frames into scratch; thread 0 then walks the
//    MONO runs, the HIGH runs (at most 3 lag frames looked at per run that passes LENGTH) and ACCEPT, in that order.
namespace {

static_assert(P3D_SHOTS_MAX_LAG <= P3D_SHOTS_CHUNK, "the carry of a chunk comes from the one chunk before it");
static_assert(CELL_WORDS <= TPB && CELL_WORDS == 3 * WAVE, "a thread a word of a cell, a wave a channel");
constexpr unsigned FLAG_CAND = 1u, FLAG_MONO = 2u, FLAG_HIGH = 4u, MARK_FADE = 1u, MARK_DISS = 2u;

__device__ __forceinline__ unsigned absdiff(unsigned p, unsigned q) { return p > q ? p - q : q - p; }

__global__ __launch_bounds__(TPB) void shots_signals(const unsigned* tabs, int cells, int carry, int lag, unsigned long long P, uint32_t* D,
                                                     uint32_t* E, long long* v, int f0) {
    __shared__ unsigned dsum[WAVES], esum[WAVES];
    __shared__ unsigned long long wsum[WAVES];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6, c = blockIdx.x, f = f0 + c;
    const size_t words = (size_t)cells * CELL_WORDS;
    const unsigned* cur = tabs + (size_t)(carry + c) * words;
    const unsigned* prev = cur - words;
    const unsigned* back = cur - (size_t)lag * words;
    const bool has_d = f > 0, has_e = lag > 0 && f >= lag;
    unsigned d = 0u, e = 0u, nb = 0u;
    if (tid < CELL_WORDS)
        for (int t = tid; t < (int)words; t += CELL_WORDS) {
            const unsigned q = cur[t];
            nb += q;
            if (has_d) d += absdiff(prev[t], q);
            if (has_e) e += absdiff(back[t], q);
        }
    unsigned long long s1 = (unsigned long long)lane * nb, s2 = (unsigned long long)(lane * lane) * nb;
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        d += __shfl_xor(d, o);
        e += __shfl_xor(e, o);
        s1 += __shfl_xor(s1, o);
        s2 += __shfl_xor(s2, o);
    }
    if (lane == 0) {
        const unsigned long long q = s1 / P, r = s1 - q * P;    // floor(S1^2 / P) = q^2 P + 2 q r + floor(r^2 / P)
        dsum[wave] = d; esum[wave] = e;
        wsum[wave] = s2 - (q * q * P + 2ull * q * r + r * r / P);
    }
    __syncthreads();
    if (tid == 0) {
        unsigned td = 0u, te = 0u;
        unsigned long long tv = 0ull;
        for (int k = 0; k < CELL_WORDS / WAVE; ++k) { td += dsum[k]; te += esum[k]; tv += wsum[k]; }
        D[f] = td; E[f] = te; v[f] = (long long)tv;
    }
}

__global__ __launch_bounds__(TPB) void shots_transitions(ShotTransitionArgs a) {
    const ShotCutArgs& c = a.cut;
    const int tid = threadIdx.x, F = c.F, K = a.lag;
    const unsigned long long floor_lhs = (unsigned long long)c.threshold_permille * 6ull * (unsigned long long)c.P;
    const unsigned long long high_lhs = (unsigned long long)a.high_permille * 6ull * (unsigned long long)c.P;
    const long long mono_rhs = (long long)a.mono_q8 * c.P;
    for (int f = tid; f < F; f += TPB) {
        unsigned is = 0u;
        if (f >= 1) {
            const unsigned long long d = c.D[f];
            unsigned nmax = 0u;
            for (int g = max(1, f - c.window); g <= min(F - 1, f + c.window); ++g)
                if (g != f) nmax = max(nmax, c.D[g]);
            if (d * 1000ull >= floor_lhs && d * 256ull >= (unsigned long long)c.ratio_q8 * nmax) is |= FLAG_CAND;
        }
        if (a.v[f] * 256ll <= mono_rhs) is |= FLAG_MONO;
        if (K > 0 && f >= K && (unsigned long long)a.E[f] * 1000ull >= high_lhs) is |= FLAG_HIGH;
        c.cand[f] = is;
        a.marks[f] = 0u;
    }
    __syncthreads();                                        // one block: its own stores to cand and marks are visible behind the barrier
    if (tid != 0) return;
    const unsigned* flag = c.cand;
    if (a.mono_min > 0) {                                   // FADE: the run [f - run, f - 1] ends before a frame f <= F - 1
        int run = 0;
        for (int f = 0; f < F; ++f) {
            if (flag[f] & FLAG_MONO) { ++run; continue; }
            if (run >= a.mono_min && f - run >= 1) a.marks[f] |= MARK_FADE;
            run = 0;
        }
    }
    for (int f = K; K > 0 && f < F;) {                      // DISS: the runs [p, q] of HIGH
        if (!(flag[f] & FLAG_HIGH)) { ++f; continue; }
        const int p = f;
        while (f < F && (flag[f] & FLAG_HIGH)) ++f;
        const int q = f - 1, n = q - p + 1;
        if (2 * n < K || n > 2 * K) continue;
        bool ok = true;
        for (int g = max(1, p - K + 1); g <= q && ok; ++g) ok = !(flag[g] & FLAG_CAND);
        const int lo = max(p - K, 0);
        long long vmin = a.v[lo];
        for (int g = lo; g <= q && ok; ++g) {
            ok = !(flag[g] & FLAG_MONO);
            vmin = min(vmin, a.v[g]);
        }
        if (ok && vmin * 256ll <= (long long)a.dip_q8 * min(a.v[lo], a.v[q])) a.marks[(p + q - K + 1) >> 1] |= MARK_DISS;
    }
    int last = 0, count = 1;
    if (c.cap > 0) { c.starts[0] = 0; a.kinds[0] = P3D_SHOT_FIRST; }
    for (int f = 1; f < F; ++f) {
        const int kind = (flag[f] & FLAG_CAND) ? P3D_SHOT_CUT : (a.marks[f] & MARK_FADE) ? P3D_SHOT_FADE : (a.marks[f] & MARK_DISS) ? P3D_SHOT_DISSOLVE : P3D_SHOT_FIRST;
        if (kind != P3D_SHOT_FIRST && f - last >= c.min_length && F - f >= c.min_length) {
            if (count < c.cap) { c.starts[count] = f; a.kinds[count] = kind; }
            ++count;
            last = f;
        }
    }
    *c.n_shots = count;
}

bool lag_ok(int lag) { return lag == 0 || (lag >= 2 && lag <= P3D_SHOTS_MAX_LAG); }

}  // namespace

TransitionsPlan p3d_transitions_plan(int gy, int gx, int n, int lag) {
    TransitionsPlan p;
    p.tables = std::min(n, P3D_SHOTS_CHUNK) + std::max(lag, 1);
    p.scratch_bytes = (long long)p.tables * gy * gx * CELL_WORDS * 4;
    return p;
}

hipError_t p3d_shot_signals_launch(const ShotSignalsArgs& a, hipStream_t s) {
    const ShotsArgs& k = a.cut;
    if (!k.frames || !k.D || !a.E || !a.v || !k.tabs || !shape_ok(k.n, k.H, k.W, k.gy, k.gx) || !lag_ok(a.lag)) return hipErrorInvalidValue;
    const ShotsPlan p = p3d_shots_plan(k.H, k.W, k.gy, k.gx, k.n);
    if (k.rows_per_block != p.rows_per_block || k.blocks_per_frame != p.blocks_per_frame || k.frames_per_chunk != p.frames_per_chunk)
        return hipErrorInvalidValue;
    const size_t T = (size_t)p.table_words;
    const int carry = std::max(a.lag, 1);
    CountArgs c;                                            // as p3d_shots_launch fills it; the count puts frame c of a chunk at slot c + 1 of its tabs
    c.frames = k.frames; c.tabs = k.tabs + (size_t)(carry - 1) * T; c.H = k.H; c.W = k.W; c.gy = k.gy; c.gx = k.gx; c.rows_per_block = p.rows_per_block;
    for (int r = 0; r <= MAX_GRID; ++r) { c.by[r] = k.H; c.nb[r] = p.blocks_per_frame; }
    int blocks = 0;
    for (int r = 0; r < k.gy; ++r) {
        c.by[r] = ceil_div((long long)r * k.H, k.gy);
        c.nb[r] = blocks;
        blocks += ceil_div(ceil_div((long long)(r + 1) * k.H, k.gy) - c.by[r], p.rows_per_block);
    }
    for (int j = 1; j < MAX_GRID; ++j) c.bx[j - 1] = j < k.gx ? ceil_div((long long)j * k.W, k.gx) : INT32_MAX;
    for (int f0 = 0; f0 < k.n; f0 += p.frames_per_chunk) {
        const int m = std::min(p.frames_per_chunk, k.n - f0);
        hipError_t e = hipMemsetAsync(k.tabs + (size_t)carry * T, 0, (size_t)m * T * sizeof(unsigned), s);
        if (e != hipSuccess) return e;
        const dim3 grid((unsigned)p.blocks_per_frame, (unsigned)m);
        if (k.ballot) hipLaunchKernelGGL(shots_count<true>, grid, dim3(TPB), 0, s, c, f0);
        else hipLaunchKernelGGL(shots_count<false>, grid, dim3(TPB), 0, s, c, f0);
        hipLaunchKernelGGL(shots_signals, dim3((unsigned)m), dim3(TPB), 0, s, (const unsigned*)k.tabs, k.gy * k.gx, carry, a.lag,
                           (unsigned long long)k.H * (unsigned long long)k.W, k.D, a.E, a.v, f0);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (f0 + m < k.n) {                                 // m is a whole chunk here, at least carry: its last carry tables seed the next
            e = hipMemcpyAsync(k.tabs, k.tabs + (size_t)m * T, (size_t)carry * T * sizeof(unsigned), hipMemcpyDeviceToDevice, s);
            if (e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

hipError_t p3d_shot_transitions_launch(const ShotTransitionArgs& a, hipStream_t s) {
    const ShotCutArgs& c = a.cut;
    if (!c.D || !a.E || !a.v || !c.cand || !a.marks || !c.n_shots || c.F < 1 || c.F > 65535 || c.P < 1 || c.P > P3D_SHOTS_MAX_PIXELS || c.cap < 0 ||
        (c.cap > 0 && (!c.starts || !a.kinds)))
        return hipErrorInvalidValue;
    if (c.threshold_permille < 1 || c.threshold_permille > 1000 || c.window < 0 || c.window > 32 || c.ratio_q8 < 256 || c.ratio_q8 > 65535 ||
        c.min_length < 1)
        return hipErrorInvalidValue;
    if (!lag_ok(a.lag) || a.high_permille < 1 || a.high_permille > 1000 || a.dip_q8 < 1 || a.dip_q8 > 256 || a.mono_q8 < 0 || a.mono_q8 > 65535 ||
        a.mono_min < 0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(shots_transitions, dim3(1), dim3(TPB), 0, s, a);
    return hipGetLastError();
}
