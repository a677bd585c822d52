// Frames low-pass filtered away from their saliency (p3d_video_prefilter, p3d_prefilter_u8; PrefilterArgs in p3d_kernels.h, the law
// in include/p3d_hip.h, "Pre-filtering frames by their 8-bit maps"): per frame the strength grid g [Hb][Wb] that qpmap.hip's
// launches leave, frame [H][W][3] bytes, out [H][W][3] bytes.  Integer arithmetic throughout and no atomics: no order can show.
//
// A rounded box pass is a launch of its own, through memory (PrefilterPlan::fused = 0 for every radius and pass count: a launch
// boundary is the fence between a pass and the halo the next one reads); the last pass blends in the same launch.  Frames go
// frames_per_chunk at a time, so that the one or two intermediate frames of a chunk stay bounded.
//  * prefilter_pass: grid (tiles_x * tiles_y, frames of the chunk), a block a TILE of PREFILTER_TILE_ROWS x PREFILTER_TILE_COLS
//    pixels, that is rows of 3 * PREFILTER_TILE_COLS interleaved bytes.
//    A  the tile's rows with a halo of R pixels come in as the aligned 16-byte words that hold them (a word that reaches outside
//       the source buffer is read byte by byte, inside only) and land in LDS at the phase they have in memory; a halo row outside
//       the frame is the border row again, a halo column outside it is clamped where it is read.
//    B  horizontal window sums, 16 bits each (<= 255 * 33): a thread slides three sums, one a channel, along 16 pixels of a row.
//    C  vertical sums of those, the exact 2-D SUM: a thread slides two neighbouring byte columns down four rows, and divides by
//       2 A with the plan's multiplier (the high word of a 32 x 32 product); the low-pass bytes go to LDS over the dead input.
//    D  a thread an aligned 16-byte word of the output row: 16 bytes from LDS, for the blend the frame's 16 bytes (two aligned
//       words and a funnel shift) and a weight a pixel from LDS, one 16-byte store; the partial words at a tile row's ends, which
//       the neighbouring tile shares, go byte by byte.
//  * What a tile skips (uniform in the block): in the last pass a tile whose grid entries are all 0 copies the frame and runs no
//    A - C; one whose entries are all 64 stores the low-pass without reading the frame.  An earlier pass p writes nothing for a
//    tile when every grid entry of the tiles within P - p tiles of it is 0: a tile of pass p + 1 that is not skipped reads only tiles
//    within one tile of itself (R <= 16 < the tile's sides), so whatever it reads was written.
#include "p3d_kernels.h"
#include "../../include/p3d_hip.h"
#include <algorithm>

namespace {

constexpr int TPB = 256;
constexpr int TH = PREFILTER_TILE_ROWS, TW = PREFILTER_TILE_COLS, MAXR = P3D_PREFILTER_MAX_RADIUS;
constexpr int TWB = 3 * TW;                               // bytes of a tile row
constexpr int IN_WORDS = (3 * (TW + 2 * MAXR) + 15 + 15) / 16;      // aligned words that hold a halo row at any phase
constexpr int IN_STRIDE = IN_WORDS * 16 + 4;              // bytes of an input row in LDS: an odd count of dwords, so rows spread over the banks
constexpr int IN_ROWS = TH + 2 * MAXR;
constexpr int H_STRIDE = TWB + 2;                         // 16-bit sums of a row: an odd count of dwords
constexpr int LOW_STRIDE = TWB + 4;                       // low-pass bytes of a row (over the input's LDS): an odd count of dwords
constexpr int IN_BYTES = IN_ROWS * IN_STRIDE, H_BYTES = IN_ROWS * H_STRIDE * 2;
constexpr int SEG = 16;                                   // pixels a thread slides along in B
constexpr int VROWS = 4;                                  // rows a thread slides down in C
constexpr int OUT_WORDS = TWB / 16 + 1;                   // aligned words that hold a tile row of the output at any phase
constexpr int GT_ROWS = TH / 8 + 2, GT_COLS = TW / 8 + 2; // grid entries a tile's pixels interpolate between, at the smallest block
static_assert(IN_STRIDE % 8 == 4 && H_STRIDE % 4 == 2 && LOW_STRIDE % 8 == 4, "odd dword strides");
static_assert(TH * LOW_STRIDE <= IN_BYTES && TH * TW * 4 <= H_BYTES, "the low-pass bytes and the weights reuse the input's and the sums' LDS");
static_assert(TW % SEG == 0 && TH % VROWS == 0 && TWB % 16 == 0 && MAXR < TH && MAXR < TW, "tile shape");
static_assert(IN_BYTES + H_BYTES <= 64 * 1024, "static LDS");

enum { MODE_LOW = 0, MODE_BLEND = 1, MODE_COPY = 2 };

__device__ __forceinline__ unsigned dword_of(const uint4& v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }

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

// The 16 bytes from address p on, all of them inside [base, end)
__device__ __forceinline__ uint4 load16(uintptr_t p, uintptr_t base, uintptr_t end) {
    const unsigned phase = (unsigned)(p & 15);
    const uintptr_t w0 = p - phase;
    const uint4 lo = word_at(w0, base, end);
    uint4 hi = make_uint4(0u, 0u, 0u, 0u);
    if (phase) hi = word_at(w0 + 16, base, end);
    const unsigned k = phase >> 2, bits = (phase & 3u) * 8u;      // whole dwords first, then bits
    const unsigned d[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    unsigned t[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) t[j] = k == 0 ? d[j] : k == 1 ? d[j + 1] : k == 2 ? d[j + 2] : d[j + 3];
    return make_uint4(__funnelshift_r(t[0], t[1], bits), __funnelshift_r(t[1], t[2], bits), __funnelshift_r(t[2], t[3], bits),
                      __funnelshift_r(t[3], t[4], bits));
}

// floor(u / 2^s) and the grid entries the pixels lo .. hi - 1 of an axis interpolate between: first .. last, not yet clamped
__device__ __forceinline__ int cell_of(int p, int B, int sh) { return (2 * p + 1 - B) >> (sh + 1); }

// Whether the grid entries that the pixels of rows [ya, yb) x columns [xa, xb) of frame m read hold a value other than 0 (x) and
// other than 64 (y), in every thread
__device__ __forceinline__ int2 grid_scan(const PrefilterArgs& a, int m, int ya, int yb, int xa, int xb, int sh) {
    const int B = a.block;
    const int ja = max(0, cell_of(ya, B, sh)), jb = min(a.Hb - 1, cell_of(yb - 1, B, sh) + 1);
    const int ia = max(0, cell_of(xa, B, sh)), ib = min(a.Wb - 1, cell_of(xb - 1, B, sh) + 1);
    const int nj = jb - ja + 1, ni = ib - ia + 1;
    const int32_t* g = a.grid + (size_t)m * (size_t)a.Hb * (size_t)a.Wb;
    int nz = 0, n64 = 0;
    for (int e = threadIdx.x; e < nj * ni; e += TPB) {
        const int j = ja + e / ni, i = ia + e % ni;
        const int v = g[(size_t)j * a.Wb + i];
        nz |= v != 0; n64 |= v != 64;
    }
    nz = __syncthreads_or(nz);
    n64 = __syncthreads_or(n64);
    return make_int2(nz, n64);
}

// pass: 1 .. P.  src [frames of the buffer][H][W][3], read for frame ms of it; dst likewise, written for frame md; m: the frame of
// the call (grid, frames).  src_frames: how many frames src holds, the bound of its word loads.
__global__ __launch_bounds__(TPB) void prefilter_pass(PrefilterArgs a, int pass, int m0, const unsigned char* src, int src_first,
                                                      int src_frames, unsigned char* dst, int dst_first) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[IN_BYTES + H_BYTES];
    __shared__ int gt[GT_ROWS * GT_COLS];
    unsigned char* const in = lds;
    unsigned short* const hs = reinterpret_cast<unsigned short*>(lds + IN_BYTES);
    unsigned char* const lowb = lds;                       // over `in`, once B has read it
    int* const wq = reinterpret_cast<int*>(lds + IN_BYTES);      // over `hs`, once C has read it
    const int tid = threadIdx.x, mm = (int)blockIdx.y, m = m0 + mm;
    const int ty = (int)(blockIdx.x / (unsigned)a.tiles_x), tx = (int)(blockIdx.x % (unsigned)a.tiles_x);
    const int y0 = ty * TH, x0 = tx * TW, R = a.radius, B = a.block, sh = __ffs(B) - 1;
    const int rows = min(TH, a.H - y0), cols = min(TW, a.W - x0), len = 3 * cols;
    const bool last = pass == a.passes;
    const size_t frame_bytes = (size_t)a.H * (size_t)a.W * 3;

    // what the tile may skip
    const int d = a.passes - pass;
    const int2 seen = grid_scan(a, m, max(0, y0 - d * TH), min(a.H, y0 + (d + 1) * TH), max(0, x0 - d * TW), min(a.W, x0 + (d + 1) * TW), sh);
    if (!seen.x && !last) return;
    const int mode = !last ? MODE_LOW : !seen.x ? MODE_COPY : !seen.y ? MODE_LOW : MODE_BLEND;

    if (mode != MODE_COPY) {
        // A: rows y0 - R .. y0 + TH - 1 + R (clamped), columns xa .. xb - 1
        const int xa = max(0, x0 - R), xb = min(a.W, x0 + TW + R), in_rows = TH + 2 * R;
        const uintptr_t sbase = (uintptr_t)src, send = sbase + (size_t)src_frames * frame_bytes;
        const uintptr_t sframe = sbase + (size_t)(m - src_first) * frame_bytes;
        const int in_len = 3 * (xb - xa);
        for (int e = tid; e < in_rows * IN_WORDS; e += TPB) {
            const int r = e / IN_WORDS, wi = e - r * IN_WORDS;
            const int gy = min(max(y0 - R + r, 0), a.H - 1);
            const uintptr_t p = sframe + ((size_t)gy * (size_t)a.W + (size_t)xa) * 3, w = (p & ~(uintptr_t)15) + (uintptr_t)wi * 16;
            if (w >= p + (uintptr_t)in_len) continue;         // past the row's last byte
            const uint4 v = word_at(w, sbase, send);
            unsigned* const to = reinterpret_cast<unsigned*>(in + r * IN_STRIDE + wi * 16);
            to[0] = v.x; to[1] = v.y; to[2] = v.z; to[3] = v.w;
        }
        __syncthreads();
        // B: hs[r][3 t + k], the sum over |dx| <= R of channel k of row r at column clamp(x0 + t + dx)
        for (int e = tid; e < in_rows * (TW / SEG); e += TPB) {
            const int seg = e / in_rows, r = e - seg * in_rows;
            const int gy = min(max(y0 - R + r, 0), a.H - 1);
            const unsigned phase = (unsigned)((sframe + ((size_t)gy * (size_t)a.W + (size_t)xa) * 3) & 15);
            const unsigned char* const row = in + r * IN_STRIDE + phase - 3 * xa;      // byte 3 x + k of the frame's row at row[3 x + k]
            const int x = x0 + seg * SEG, xm = a.W - 1;
            unsigned s0 = 0u, s1 = 0u, s2 = 0u;
            for (int dx = -R; dx <= R; ++dx) {
                const unsigned char* q = row + 3 * min(max(x + dx, 0), xm);
                s0 += q[0]; s1 += q[1]; s2 += q[2];
            }
            unsigned* const to = reinterpret_cast<unsigned*>(hs + r * H_STRIDE + 3 * seg * SEG);
#pragma unroll 2
            for (int t = 0; t < SEG; t += 2) {
                const unsigned char* qa = row + 3 * min(max(x + t + R + 1, 0), xm);
                const unsigned char* ql = row + 3 * min(max(x + t - R, 0), xm);
                const unsigned n0 = s0 + qa[0] - ql[0], n1 = s1 + qa[1] - ql[1], n2 = s2 + qa[2] - ql[2];
                to[3 * (t >> 1)] = s0 | (s1 << 16); to[3 * (t >> 1) + 1] = s2 | (n0 << 16); to[3 * (t >> 1) + 2] = n1 | (n2 << 16);
                qa = row + 3 * min(max(x + t + R + 2, 0), xm);
                ql = row + 3 * min(max(x + t + 1 - R, 0), xm);
                s0 = n0 + qa[0] - ql[0]; s1 = n1 + qa[1] - ql[1]; s2 = n2 + qa[2] - ql[2];
            }
        }
        __syncthreads();
        // C: lowb[y][c], c = 2 cp and 2 cp + 1
        const unsigned A = (unsigned)((2 * R + 1) * (2 * R + 1));
        const unsigned* const h32 = reinterpret_cast<const unsigned*>(hs);
        for (int e = tid; e < (TH / VROWS) * (TWB / 2); e += TPB) {
            const int rs = e / (TWB / 2), cp = e - rs * (TWB / 2), y = rs * VROWS;
            const unsigned* const hp = h32 + cp;
            unsigned sa = 0u, sb = 0u;
            for (int r = y; r <= y + 2 * R; ++r) {
                const unsigned v = hp[r * (H_STRIDE / 2)];
                sa += v & 0xffffu; sb += v >> 16;
            }
#pragma unroll
            for (int j = 0; j < VROWS; ++j) {
                const unsigned la = __umulhi(2u * sa + A, a.mul), lb = __umulhi(2u * sb + A, a.mul);
                *reinterpret_cast<unsigned short*>(lowb + (y + j) * LOW_STRIDE + 2 * cp) = (unsigned short)(la | (lb << 8));
                if (j + 1 < VROWS) {
                    const unsigned vn = hp[(y + j + 2 * R + 1) * (H_STRIDE / 2)], vo = hp[(y + j) * (H_STRIDE / 2)];
                    sa += (vn & 0xffffu) - (vo & 0xffffu); sb += (vn >> 16) - (vo >> 16);
                }
            }
        }
        // (lowb lies over `in`, which B has read: the barrier between B and C stands between them)
    }
    if (mode == MODE_BLEND) {
        // the grid entries the tile's pixels interpolate between, then a weight a pixel (over hs: behind C)
        const int j_lo = cell_of(y0, B, sh), i_lo = cell_of(x0, B, sh);
        const int32_t* g = a.grid + (size_t)m * (size_t)a.Hb * (size_t)a.Wb;
        for (int e = tid; e < GT_ROWS * GT_COLS; e += TPB) {
            const int j = min(max(j_lo + e / GT_COLS, 0), a.Hb - 1), i = min(max(i_lo + e % GT_COLS, 0), a.Wb - 1);
            gt[e] = g[(size_t)j * a.Wb + i];
        }
        __syncthreads();                                       // gt is written, and C has read hs
        const int D = 2 * B;
        for (int e = tid; e < TH * TW; e += TPB) {
            const int yy = e / TW, xx = e - yy * TW;
            const int u = 2 * (y0 + yy) + 1 - B, v = 2 * (x0 + xx) + 1 - B;
            const int j = (u >> (sh + 1)) - j_lo, fy = u & (D - 1), i = (v >> (sh + 1)) - i_lo, fx = v & (D - 1);
            const int* const c = gt + j * GT_COLS + i;
            wq[e] = (D - fy) * ((D - fx) * c[0] + fx * c[1]) + fy * ((D - fx) * c[GT_COLS] + fx * c[GT_COLS + 1]);
        }
    }
    __syncthreads();
    // D: the tile's rows as aligned 16-byte words of dst
    const int lq = 8 + 2 * sh;
    const unsigned Q = 1u << lq;
    const uintptr_t fbase = (uintptr_t)a.frames, fend = fbase + (size_t)a.n * frame_bytes;
    for (int e = tid; e < rows * OUT_WORDS; e += TPB) {
        const int yy = e / OUT_WORDS, wi = e - yy * OUT_WORDS;
        const size_t at = ((size_t)(y0 + yy) * (size_t)a.W + (size_t)x0) * 3;      // the tile row's first byte inside a frame
        const uintptr_t po = (uintptr_t)dst + (size_t)(m - dst_first) * frame_bytes + at;
        const uintptr_t pf = fbase + (size_t)m * frame_bytes + at;
        const long long b0 = (long long)((po & ~(uintptr_t)15) + (uintptr_t)wi * 16) - (long long)po;      // the word's first byte in the tile row: -15 .. len + 14
        if (b0 >= len) continue;
        const bool whole = b0 >= 0 && b0 + 16 <= len;
        uint4 vf = make_uint4(0u, 0u, 0u, 0u);
        if (mode != MODE_LOW && whole) vf = load16(pf + (uintptr_t)b0, fbase, fend);
        unsigned o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int b = (int)b0 + j;
            if (!whole && (b < 0 || b >= len)) continue;
            unsigned f = 0u, v;
            if (mode != MODE_LOW) f = whole ? (dword_of(vf, j >> 2) >> ((j & 3) * 8)) & 255u : (unsigned)*reinterpret_cast<const unsigned char*>(pf + b);
            if (mode == MODE_COPY) v = f;
            else {
                v = lowb[yy * LOW_STRIDE + b];
                if (mode == MODE_BLEND) {
                    const unsigned wn = (unsigned)wq[yy * TW + (int)(((unsigned)b * 21846u) >> 16)];      // b / 3 for b < 2^15
                    v = (f * (Q - wn) + v * wn + (Q >> 1)) >> lq;
                }
            }
            if (whole) o[j >> 2] |= v << ((j & 3) * 8);
            else *reinterpret_cast<unsigned char*>(po + b) = (unsigned char)v;
        }
        if (whole) *reinterpret_cast<uint4*>(po + (uintptr_t)b0) = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

bool block_ok(int B) { return B == 8 || B == 16 || B == 32 || B == 64 || B == 128; }

bool args_ok(const PrefilterArgs& a) {
    if (!a.frames || !a.out || !a.grid) return false;
    if (a.n < 1 || a.n > 65535 || a.H < 1 || a.W < 1 || (long long)a.H * a.W > P3D_PREFILTER_MAX_PIXELS) return false;
    if (!block_ok(a.block) || a.radius < 1 || a.radius > MAXR || a.passes < 1 || a.passes > P3D_PREFILTER_MAX_PASSES) return false;
    if ((a.passes > 1 && !a.tmp[0]) || (a.passes > 2 && !a.tmp[1])) return false;
    const PrefilterPlan p = p3d_prefilter_plan(a.H, a.W, a.block, a.radius, a.passes, a.n);
    return a.Hb == p.Hb && a.Wb == p.Wb && a.tiles_x == p.tiles_x && a.tiles_y == p.tiles_y && a.frames_per_chunk == p.frames_per_chunk &&
           a.mul == p.mul && a.shift == p.shift;
}

}  // namespace

PrefilterPlan p3d_prefilter_plan(int H, int W, int block, int radius, int passes, int n) {
    PrefilterPlan p;
    if (!block_ok(block) || radius < 1 || radius > MAXR || passes < 1 || passes > P3D_PREFILTER_MAX_PASSES) return p;
    p.Hb = (H + block - 1) / block; p.Wb = (W + block - 1) / block;
    p.tile_rows = TH; p.tile_cols = TW; p.halo = radius; p.fused = 0;
    p.tiles_x = (W + TW - 1) / TW; p.tiles_y = (H + TH - 1) / TH;
    p.blocks_per_frame = (long long)p.tiles_x * p.tiles_y;
    const long long frame_bytes = (long long)H * W * 3;
    p.frames_per_chunk = passes == 1 ? n : (int)std::max<long long>(1, std::min<long long>(n, P3D_PREFILTER_CHUNK_BYTES / frame_bytes));
    p.tmp_bytes = passes == 1 ? 0 : (p.frames_per_chunk * frame_bytes + 255) & ~255LL;      // from a 256-byte boundary
    p.scratch_bytes = p.tmp_bytes * std::min(passes - 1, 2);
    // floor(x / (2 A)) = (x * mul) >> 32 for every x < 2^20 >= 2 * 255 * A + A: mul = ceil(2^(20 + l) / (2 A)) with l = 12 >= log2(2 A)
    const unsigned long long den = 2ULL * (2 * radius + 1) * (2 * radius + 1);
    p.mul = (unsigned)(((1ULL << 32) + den - 1) / den); p.shift = 32;
    return p;
}

hipError_t p3d_prefilter_launch(const PrefilterArgs& a, hipStream_t s) {
    if (!args_ok(a)) return hipErrorInvalidValue;
    const unsigned tiles = (unsigned)(a.tiles_x * a.tiles_y);
    for (int m0 = 0; m0 < a.n; m0 += a.frames_per_chunk) {
        const int c = std::min(a.frames_per_chunk, a.n - m0);
        for (int pass = 1; pass <= a.passes; ++pass) {
            // pass 1 reads the frames; pass p > 1 the intermediate pass p - 1 wrote, the two taking turns
            const unsigned char* src = pass == 1 ? a.frames : a.tmp[(pass - 2) & 1];
            unsigned char* dst = pass == a.passes ? a.out : a.tmp[(pass - 1) & 1];
            hipLaunchKernelGGL(prefilter_pass, dim3(tiles, (unsigned)c), dim3(TPB), 0, s, a, pass, m0, src, pass == 1 ? 0 : m0,
                               pass == 1 ? a.n : c, dst, pass == a.passes ? 0 : m0);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
