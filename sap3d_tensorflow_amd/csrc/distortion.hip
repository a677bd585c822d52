// Distortion of frames under their 8-bit maps (p3d_video_distortion, p3d_distortion_u8; DistortionArgs in p3d_kernels.h, the law in
// include/p3d_hip.h, "Distortion of frames under their 8-bit maps"): per frame s [H][W] bytes, ref and test [H][W][3] bytes ->
// table [P3D_DISTORTION_RECORD] int64 and the optional block_sse [Hb][Wb] int64.  Integers throughout but for SSIM's one division,
// whose quotient is quantised before it is summed; every cross-block combination is a 64-bit integer atomic at agent scope (add, or
// max for MAXABS) into outputs that p3d_distortion_launch zeroes first, so no order can show.
//  * distortion_sums: grid (tiles_x * tiles_y, n), a block a tile of DISTORTION_TILE_ROWS x DISTORTION_TILE_COLS pixels.  A lane
//    owns 16 pixels of a row, twice (rows r and r + 32 of the tile): s comes in as the 16 bytes that hold them, ref and test as their
//    48 bytes, each from the aligned 16-byte words that hold them and a funnel shift by the base's phase (a word that reaches
//    outside the buffer is read byte by byte, inside only).  The weight law sits in LDS as bytes.  Per-lane partials are 32 bits wide
//    (the bound stands beside them), WSSE widens to 64 bits before the wave's fold, the four waves meet in LDS, and one thread a
//    field adds to the table.  The block map's squared differences fold in LDS, a cell a block (or the tile's part of one), and go
//    out with one atomic a cell.
//  * distortion_ssim: grid (ssim_tiles_x * ssim_tiles_y, n), a block the windows whose top-left 4 x 4 cell lies in its tile of
//    DISTORTION_SSIM_ROWS x DISTORTION_SSIM_COLS pixels: 8 x 16 windows.  Y of both frames is computed on the fly; a lane takes 16
//    pixels of one of the tile's 36 rows (one cell of halo below and to the right) and leaves six sums per cell row in LDS (a, b,
//    aa, bb, ab of the Y values, and w); a window is the sum of the 4 rows of its 2 x 2 cells.  Only cells wholly inside the frame
//    are summed: a window that exists reads no other.
#include "p3d_kernels.h"
#include "../../include/p3d_hip.h"
#include <algorithm>

namespace {

constexpr int TPB = 256, WAVE = 64, WAVES = TPB / WAVE;
constexpr int TH = DISTORTION_TILE_ROWS, TW = DISTORTION_TILE_COLS, SEG = 16;
constexpr int SEGS = TW / SEG, LANE_ROWS = TH / (TPB / SEGS);      // segments of a tile row; rows a lane takes
constexpr int BCELLS = (TH / 8) * (TW / 8);                        // the block map's cells of a tile at the smallest block
constexpr int SH = DISTORTION_SSIM_ROWS, SW_ = DISTORTION_SSIM_COLS;
constexpr int CROWS = SH / 4 + 1, CCOLS = SW_ / 4 + 1;             // 4 x 4 cells of a tile with its halo
constexpr int PROWS = 4 * CROWS, PSEGS = (4 * CCOLS + SEG - 1) / SEG;      // pixel rows, and 16-pixel segments of one
constexpr int NSUM = 6;                                            // a, b, aa, bb, ab, w
constexpr int FIELDS = 16;                                         // the record's fields the sums' launch makes: SSE .. CHANGED_SALIENT
static_assert(TPB % SEGS == 0 && TH % (TPB / SEGS) == 0 && TW % SEG == 0, "tile shape");
// A lane's 32-bit partials: LANE_ROWS * 16 pixels of at most 255 * 255^2 each (WSSE, the largest).  259 pixels would overflow.
static_assert((unsigned long long)LANE_ROWS * SEG * 255ULL * 65025ULL < (1ULL << 32), "a lane's WSSE partial fits 32 bits");
// A wave's 32-bit folds (everything but WSSE): 64 lanes of at most LANE_ROWS * 16 * 65025 each
static_assert((unsigned long long)WAVE * LANE_ROWS * SEG * 65025ULL < (1ULL << 32), "a wave's SSE fits 32 bits");
// A cell of the block map in LDS: at most the whole tile, 3 * 255^2 a pixel
static_assert((unsigned long long)TH * TW * 3ULL * 65025ULL < (1ULL << 32), "a tile's squared differences fit 32 bits");
static_assert(PROWS * PSEGS <= TPB && (SH / 4) * (SW_ / 4) <= TPB, "a thread a row segment, a thread a window");
static_assert(P3D_DISTORTION_SSE == 0 && P3D_DISTORTION_WSSE == 4 && P3D_DISTORTION_SW == 8 && P3D_DISTORTION_MAXABS == 9 &&
              P3D_DISTORTION_CHANGED == 13 && P3D_DISTORTION_SALIENT == 14 && P3D_DISTORTION_CHANGED_SALIENT == 15, "the record's order");

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

// The 16 NW bytes from address p on into o: NW + 1 aligned words (NW when p is aligned) and a funnel shift by p's phase.  Bytes
// outside [base, end) read as 0.
template <int NW>
__device__ __forceinline__ void load_bytes(uintptr_t p, uintptr_t base, uintptr_t end, unsigned (&o)[4 * NW]) {
    const unsigned phase = (unsigned)(p & 15);
    const uintptr_t w0 = p - phase;
    unsigned d[4 * NW + 4];
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        const uint4 v = word_at(w0 + 16u * j, base, end);
        d[4 * j] = v.x; d[4 * j + 1] = v.y; d[4 * j + 2] = v.z; d[4 * j + 3] = v.w;
    }
    uint4 hi = make_uint4(0u, 0u, 0u, 0u);
    if (phase) hi = word_at(w0 + 16u * NW, base, end);
    d[4 * NW] = hi.x; d[4 * NW + 1] = hi.y; d[4 * NW + 2] = hi.z; d[4 * NW + 3] = hi.w;
    const unsigned k = phase >> 2, bits = (phase & 3u) * 8u;      // whole dwords first, then bits
    unsigned t[4 * NW + 1];
#pragma unroll
    for (int j = 0; j <= 4 * NW; ++j) t[j] = k == 0 ? d[j] : k == 1 ? d[j + 1] : k == 2 ? d[j + 2] : d[j + 3];
#pragma unroll
    for (int j = 0; j < 4 * NW; ++j) o[j] = __funnelshift_r(t[j], t[j + 1], bits);
}

__device__ __forceinline__ unsigned byte_of(const unsigned* o, int b) { return (o[b >> 2] >> ((b & 3) * 8)) & 255u; }
__device__ __forceinline__ unsigned luma(unsigned b, unsigned g, unsigned r) { return (29u * b + 150u * g + 77u * r + 128u) >> 8; }
__device__ __forceinline__ unsigned absdiff(unsigned x, unsigned y) { return x > y ? x - y : y - x; }

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
    for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned wave_max(unsigned v) {
    for (int o = WAVE / 2; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ long long wave_sum64(long long v) {
    for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ void lds_add(unsigned* at, unsigned v) { __hip_atomic_fetch_add(at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void table_add(long long* at, long long v) {
    if (v) __hip_atomic_fetch_add(at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(TPB) void distortion_sums(DistortionArgs a) {
    __shared__ unsigned char lw[256];
    __shared__ unsigned bl[BCELLS];
    __shared__ unsigned long long part[WAVES][FIELDS];
    const int tid = threadIdx.x, m = (int)blockIdx.y;
    const int ty = (int)(blockIdx.x / (unsigned)a.tiles_x), tx = (int)(blockIdx.x % (unsigned)a.tiles_x);
    const int y0 = ty * TH, x0 = tx * TW;
    lw[tid] = (unsigned char)a.wlaw[tid];
    if (tid < BCELLS) bl[tid] = 0u;
    __syncthreads();

    const size_t pixels = (size_t)a.H * (size_t)a.W;
    const uintptr_t sbase = (uintptr_t)a.sal, send = sbase + (size_t)a.n * pixels;
    const uintptr_t rbase = (uintptr_t)a.ref, rend = rbase + (size_t)a.n * pixels * 3;
    const uintptr_t tbase = (uintptr_t)a.test, tend = tbase + (size_t)a.n * pixels * 3;
    const int seg = tid % SEGS, row = tid / SEGS, xs = x0 + seg * SEG;
    const int bsh = a.block ? __ffs(a.block) - 1 : 0;
    const unsigned gate = (unsigned)a.gate;

    // a lane's partials, 32 bits each: see the bounds above
    unsigned sse[4] = {0u, 0u, 0u, 0u}, wsse[4] = {0u, 0u, 0u, 0u}, mx[4] = {0u, 0u, 0u, 0u}, sw = 0u, changed = 0u, salient = 0u, both = 0u;
    for (int k = 0; k < LANE_ROWS; ++k) {
        const int y = y0 + row + k * (TH / LANE_ROWS);
        if (y >= a.H || xs >= a.W) continue;
        const int cnt = min(SEG, a.W - xs);
        const size_t at = (size_t)m * pixels + (size_t)y * (size_t)a.W + (size_t)xs;
        unsigned s[4], r[12], t[12];
        load_bytes<1>(sbase + at, sbase, send, s);
        load_bytes<3>(rbase + at * 3, rbase, rend, r);
        load_bytes<3>(tbase + at * 3, tbase, tend, t);
        unsigned pair[2] = {0u, 0u};                           // d_B^2 + d_G^2 + d_R^2 of pixels 0 .. 7 and 8 .. 15
#pragma unroll
        for (int j = 0; j < SEG; ++j) {
            if (j >= cnt) continue;                            // (the bytes past the row's end belong to the next row)
            const unsigned sv = byte_of(s, j), w = lw[sv];
            const unsigned rb = byte_of(r, 3 * j), rg = byte_of(r, 3 * j + 1), rr = byte_of(r, 3 * j + 2);
            const unsigned tb = byte_of(t, 3 * j), tg = byte_of(t, 3 * j + 1), tr = byte_of(t, 3 * j + 2);
            const unsigned d[4] = {absdiff(rb, tb), absdiff(rg, tg), absdiff(rr, tr), absdiff(luma(rb, rg, rr), luma(tb, tg, tr))};
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const unsigned q = d[p] * d[p];
                sse[p] += q; wsse[p] += w * q; mx[p] = max(mx[p], d[p]);
            }
            pair[j >> 3] += d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
            const unsigned ch = (d[0] | d[1] | d[2]) != 0u, sa = gate != 0u && sv >= gate;
            sw += w; changed += ch; salient += sa; both += ch & sa;
        }
        if (a.block_sse) {
            // the tile's cell of the block that holds the pixels: a tile starts on a block's boundary, or lies inside one block
            const int ly = (y >> bsh) - (y0 >> bsh), lx = (xs >> bsh) - (x0 >> bsh);
            if (a.block == 8) {
                if (pair[0]) lds_add(&bl[ly * (TW / 8) + lx], pair[0]);
                if (pair[1]) lds_add(&bl[ly * (TW / 8) + lx + 1], pair[1]);
            } else if (pair[0] + pair[1]) lds_add(&bl[ly * (TW / 8) + lx], pair[0] + pair[1]);
        }
    }

    // the wave's fold: WSSE in 64 bits, the rest in 32 (the bounds above), then the four waves through LDS
    const int lane = tid % WAVE, wv = tid / WAVE;
    unsigned long long f[FIELDS];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        f[P3D_DISTORTION_SSE + p] = wave_sum(sse[p]);
        f[P3D_DISTORTION_WSSE + p] = (unsigned long long)wave_sum64((long long)wsse[p]);
        f[P3D_DISTORTION_MAXABS + p] = wave_max(mx[p]);
    }
    f[P3D_DISTORTION_SW] = wave_sum(sw);
    f[P3D_DISTORTION_CHANGED] = wave_sum(changed);
    f[P3D_DISTORTION_SALIENT] = wave_sum(salient);
    f[P3D_DISTORTION_CHANGED_SALIENT] = wave_sum(both);
    if (lane == 0) {
#pragma unroll
        for (int p = 0; p < FIELDS; ++p) part[wv][p] = f[p];
    }
    __syncthreads();
    long long* const rec = a.table + (size_t)m * P3D_DISTORTION_RECORD;
    if (tid < FIELDS) {
        const bool is_max = tid >= P3D_DISTORTION_MAXABS && tid < P3D_DISTORTION_MAXABS + 4;
        unsigned long long v = 0ULL;
        for (int w = 0; w < WAVES; ++w) v = is_max ? max(v, part[w][tid]) : v + part[w][tid];
        if (is_max) { if (v) atomicMax(reinterpret_cast<unsigned long long*>(rec + tid), v); }
        else table_add(rec + tid, (long long)v);
    }
    if (a.block_sse) {
        const int cy = a.block >= TH ? 1 : TH >> bsh, cx = a.block >= TW ? 1 : TW >> bsh;      // the tile's cells
        if (tid < cy * cx) {
            const int ly = tid / cx, lx = tid % cx, gy = (y0 >> bsh) + ly, gx = (x0 >> bsh) + lx;
            const unsigned v = bl[ly * (TW / 8) + lx];
            if (gy < a.Hb && gx < a.Wb) table_add(a.block_sse + ((size_t)m * (size_t)a.Hb + (size_t)gy) * (size_t)a.Wb + (size_t)gx, (long long)v);
        }
    }
}

__global__ __launch_bounds__(TPB) void distortion_ssim(DistortionArgs a) {
    __shared__ unsigned char lw[256];
    __shared__ int rs[PROWS][CCOLS][NSUM];                 // per pixel row and cell: the sums of the cell's 4 pixels of that row
    __shared__ long long part[WAVES][4];
    const int tid = threadIdx.x, m = (int)blockIdx.y;
    const int ty = (int)(blockIdx.x / (unsigned)a.ssim_tiles_x), tx = (int)(blockIdx.x % (unsigned)a.ssim_tiles_x);
    const int y0 = ty * SH, x0 = tx * SW_;
    lw[tid] = (unsigned char)a.wlaw[tid];
    __syncthreads();

    const size_t pixels = (size_t)a.H * (size_t)a.W;
    if (tid < PROWS * PSEGS) {
        const int pr = tid / PSEGS, sg = tid % PSEGS, y = y0 + pr, xs = x0 + sg * SEG;
        const int cells = min(SEG / 4, CCOLS - sg * (SEG / 4));      // of this segment: 4, or 1 in the halo's
        int full = 0;                                          // its cells that lie wholly inside the frame's row
        if (y < a.H && xs < a.W) full = min(cells, (a.W - xs) / 4);
        unsigned s[4] = {0u, 0u, 0u, 0u}, r[12], t[12];
        if (full) {
            const uintptr_t sbase = (uintptr_t)a.sal, rbase = (uintptr_t)a.ref, tbase = (uintptr_t)a.test;
            const size_t at = (size_t)m * pixels + (size_t)y * (size_t)a.W + (size_t)xs;
            load_bytes<1>(sbase + at, sbase, sbase + (size_t)a.n * pixels, s);
            load_bytes<3>(rbase + at * 3, rbase, rbase + (size_t)a.n * pixels * 3, r);
            load_bytes<3>(tbase + at * 3, tbase, tbase + (size_t)a.n * pixels * 3, t);
        }
#pragma unroll
        for (int c = 0; c < SEG / 4; ++c) {
            if (c >= cells) continue;
            int v[NSUM] = {0, 0, 0, 0, 0, 0};
            if (c < full) {
#pragma unroll
                for (int j = 4 * c; j < 4 * c + 4; ++j) {
                    const int ya = (int)luma(byte_of(r, 3 * j), byte_of(r, 3 * j + 1), byte_of(r, 3 * j + 2));
                    const int yb = (int)luma(byte_of(t, 3 * j), byte_of(t, 3 * j + 1), byte_of(t, 3 * j + 2));
                    v[0] += ya; v[1] += yb; v[2] += ya * ya; v[3] += yb * yb; v[4] += ya * yb; v[5] += (int)lw[byte_of(s, j)];
                }
            }
#pragma unroll
            for (int z = 0; z < NSUM; ++z) rs[pr][sg * (SEG / 4) + c][z] = v[z];
        }
    }
    __syncthreads();

    // a thread a window: the 4 rows of its 2 x 2 cells.  64 pixels: sa, sb <= 16320, saa, sbb, sab <= 64 * 65025, ww <= 16320
    long long q = 0, wq = 0, wsum = 0, cnt = 0;
    if (tid < (SH / 4) * (SW_ / 4)) {
        const int wj = tid / (SW_ / 4), wi = tid % (SW_ / 4);
        if (y0 / 4 + wj < a.win_rows && x0 / 4 + wi < a.win_cols) {
            int v[NSUM] = {0, 0, 0, 0, 0, 0};
            for (int pr = 4 * wj; pr < 4 * wj + 8; ++pr)
#pragma unroll
                for (int z = 0; z < NSUM; ++z) v[z] += rs[pr][wi][z] + rs[pr][wi + 1][z];
            const long long sa = v[0], sb = v[1], saa = v[2], sbb = v[3], sab = v[4];
            const long long c1 = 26634, c2 = 235963;
            const long long num = (2 * sa * sb + c1) * (2 * (64 * sab - sa * sb) + c2);
            const long long den = (sa * sa + sb * sb + c1) * (64 * (saa + sbb) - sa * sa - sb * sb + c2);
            q = (long long)floor((double)num / (double)den * 65536.0 + 0.5);
            wsum = v[5]; wq = wsum * q; cnt = 1;
        }
    }
    if (tid < 2 * WAVE) {                                      // the windows' threads are the first two waves, whole
        q = wave_sum64(q); wq = wave_sum64(wq); wsum = wave_sum64(wsum); cnt = wave_sum64(cnt);
        if (tid % WAVE == 0) { part[tid / WAVE][0] = cnt; part[tid / WAVE][1] = q; part[tid / WAVE][2] = wq; part[tid / WAVE][3] = wsum; }
    }
    __syncthreads();
    if (tid < 4) table_add(a.table + (size_t)m * P3D_DISTORTION_RECORD + P3D_DISTORTION_NW + tid, part[0][tid] + part[1][tid]);
}

bool block_ok(int B) { return B == 0 || B == 8 || B == 16 || B == 32 || B == 64 || B == 128; }

bool args_ok(const DistortionArgs& a) {
    if (!a.sal || !a.ref || !a.test || !a.wlaw || !a.table) return false;
    if (a.n < 1 || a.n > 65535 || a.H < 1 || a.W < 1 || (long long)a.H * a.W > P3D_DISTORTION_MAX_PIXELS) return false;
    if (!block_ok(a.block) || a.gate < 0 || a.gate > 255 || (a.block == 0 && a.block_sse)) return false;
    const DistortionPlan p = p3d_distortion_plan(a.H, a.W, a.block, a.n);
    return a.Hb == p.Hb && a.Wb == p.Wb && a.tiles_x == p.tiles_x && a.tiles_y == p.tiles_y && a.win_rows == p.win_rows &&
           a.win_cols == p.win_cols && a.ssim_tiles_x == p.ssim_tiles_x && a.ssim_tiles_y == p.ssim_tiles_y;
}

}  // namespace

DistortionPlan p3d_distortion_plan(int H, int W, int block, int n) {
    DistortionPlan p;
    if (!block_ok(block) || H < 1 || W < 1 || n < 1) return p;
    p.Hb = block ? (H + block - 1) / block : 0; p.Wb = block ? (W + block - 1) / block : 0;
    p.tile_rows = TH; p.tile_cols = TW;
    p.tiles_x = (W + TW - 1) / TW; p.tiles_y = (H + TH - 1) / TH;
    p.blocks_per_frame = (long long)p.tiles_x * p.tiles_y;
    // a window's corner is (4 j, 4 i) with 4 j + 8 <= H and 4 i + 8 <= W
    p.win_rows = H >= 8 && W >= 8 ? (H - 8) / 4 + 1 : 0; p.win_cols = H >= 8 && W >= 8 ? (W - 8) / 4 + 1 : 0;
    p.ssim_tiles_y = (4 * p.win_rows + SH - 1) / SH; p.ssim_tiles_x = (4 * p.win_cols + SW_ - 1) / SW_;
    p.scratch_bytes = 0;
    return p;
}

hipError_t p3d_distortion_launch(const DistortionArgs& a, hipStream_t s) {
    if (!args_ok(a)) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(a.table, 0, (size_t)a.n * P3D_DISTORTION_RECORD * sizeof(long long), s);
    if (e != hipSuccess) return e;
    if (a.block_sse) {
        e = hipMemsetAsync(a.block_sse, 0, (size_t)a.n * (size_t)a.Hb * (size_t)a.Wb * sizeof(long long), s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(distortion_sums, dim3((unsigned)(a.tiles_x * a.tiles_y), (unsigned)a.n), dim3(TPB), 0, s, a);
    if (a.win_rows > 0)
        hipLaunchKernelGGL(distortion_ssim, dim3((unsigned)(a.ssim_tiles_x * a.ssim_tiles_y), (unsigned)a.n), dim3(TPB), 0, s, a);
    return hipGetLastError();
}
