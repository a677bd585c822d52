// Overlays of 8-bit saliency maps on their frames (p3d_video_render, p3d_render_u8; RenderArgs in p3d_kernels.h, the law in
// include/p3d_hip.h, "Rendering 8-bit maps"): per map saliency s [H][W] bytes, frame [H][W][3] bytes (or none), one 256-entry table
// of colour and opacity for every map, out [H][W][3] bytes.  Integer arithmetic throughout: no order can show.
//
//  * render_kernel<FRAME, false> (no contour): grid (blocks, n) -- blocks past RENDER_GRID_X fold into z --, block j of map m takes the flat run of pixels
//    [j * chunk, (j + 1) * chunk), chunk a multiple of 16.  Where s, frame and out of the run are aligned alike (RenderCut: the
//    frame and out bytes of pixel p start at 3 p, so "alike" is frame = out = 3 s modulo 16) a lane takes 16 consecutive pixels:
//    one 16-byte load of s, three of the frame, three 16-byte stores, between a head and a tail of single pixels; otherwise every
//    pixel is byte loads and stores.  7 bytes a pixel, s read once; this instantiation holds no halo code.
//  * The table is staged once per block in LDS in the form the blend needs: per level (c_b o + 127) | (c_g o + 127) << 16 and
//    (c_r o + 127) | (255 - o) << 16 (2 KB), so a channel costs one multiply-add and one division by 255; without a frame the raw
//    entries (1 KB).
//  * render_kernel<FRAME, true> (contour): grid (tiles, n), a tile of RENDER_TILE_ROWS x RENDER_TILE_COLS pixels.  The block reads
//    the tile's s with a halo of t pixels (16-byte words between single pixels, each halo row by half a wave) and keeps one BIT a
//    pixel in LDS, set where s < L; pixels outside the map stay clear, so they never count.  Two passes over those words in LDS
//    -- OR over |dx| <= t by shifts, OR over |dy| <= t by rows -- leave "some pixel of the window is below L"; a pixel is on the
//    contour where that bit is set and its own s >= L.  Every row of the tile is then rendered as a run by 16 lanes with the same
//    body as above.  The LDS atomics only merge bits inside the block; blocks share nothing.
#include "p3d_kernels.h"
#include "../../include/p3d_hip.h"
#include <algorithm>

namespace {

constexpr int TPB = 256;
constexpr int TR = RENDER_TILE_ROWS, TC = RENDER_TILE_COLS;
constexpr int MAXT = P3D_RENDER_MAX_THICKNESS;
constexpr int HALO_ROWS = TR + 2 * MAXT;
constexpr int ROW_WORDS = (TC + 2 * MAXT + 31) / 32 + 1;      // one word more: 16 bits are taken from two words at any position
static_assert(HALO_ROWS * ROW_WORDS <= TPB, "one thread per word in the two LDS passes");
static_assert(TC / 16 * TR == TPB, "16 lanes a row, every row of the tile at once");
static_assert((TC + 2 * MAXT + 15) / 16 + 2 <= 32, "a halo row's words fit half a wave");


__device__ __forceinline__ unsigned dword_of(const uint4& v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }
__device__ __forceinline__ unsigned byte_of(const uint4& v, int j) { return (dword_of(v, j >> 2) >> ((j & 3) * 8)) & 255u; }

// one pixel: level s, frame bytes f[3] -> o[3]
template <bool FRAME>
__device__ __forceinline__ void shade(const unsigned* lds, unsigned s, const unsigned f[3], bool contour, unsigned cc, unsigned o[3]) {
    if (FRAME) {
        const unsigned c01 = lds[2 * s], c2w = lds[2 * s + 1], w = c2w >> 16;
        o[0] = (f[0] * w + (c01 & 0xffffu)) / 255u;
        o[1] = (f[1] * w + (c01 >> 16)) / 255u;
        o[2] = (f[2] * w + (c2w & 0xffffu)) / 255u;
    } else {
        const unsigned e = lds[s];
        o[0] = e & 255u; o[1] = (e >> 8) & 255u; o[2] = (e >> 16) & 255u;
    }
    if (contour) { o[0] = cc & 255u; o[1] = (cc >> 8) & 255u; o[2] = (cc >> 16) & 255u; }
}

// 16 bits of a row of LDS words from bit position p
__device__ __forceinline__ unsigned bits16(const unsigned* row, int p) {
    const unsigned long long two = (unsigned long long)row[p >> 5] | ((unsigned long long)row[(p >> 5) + 1] << 32);
    return (unsigned)(two >> (p & 31)) & 0xffffu;
}

// A run of len consecutive pixels by nl lanes (this one is li): ps / pf / po the run's first bytes.  CONTOUR: bit cb + i of crow is
// "some pixel of pixel i's window is below L".
template <bool FRAME, bool CONTOUR>
__device__ __forceinline__ void render_run(const unsigned* lds, const unsigned char* ps, const unsigned char* pf, unsigned char* po, int len,
                                           int li, int nl, unsigned level, unsigned cc, const unsigned* crow, int cb) {
    const RenderCut cut = p3d_render_cut((uintptr_t)ps, FRAME ? (uintptr_t)pf : 3 * (uintptr_t)ps, (uintptr_t)po, len);
    const uint4* s4 = reinterpret_cast<const uint4*>(ps + cut.head);
    const uint4* f4 = reinterpret_cast<const uint4*>(pf + 3 * cut.head);
    uint4* o4 = reinterpret_cast<uint4*>(po + 3 * cut.head);
    for (int q = li; q < cut.words; q += nl) {
        const uint4 vs = s4[q];
        uint4 vf[3];
        if (FRAME) { vf[0] = f4[3 * q]; vf[1] = f4[3 * q + 1]; vf[2] = f4[3 * q + 2]; }
        const unsigned near = CONTOUR ? bits16(crow, cb + cut.head + 16 * q) : 0u;
        unsigned w[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) w[k] = 0u;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const unsigned s = byte_of(vs, j);
            unsigned f[3] = {0u, 0u, 0u}, o[3];
            if (FRAME) {
#pragma unroll
                for (int k = 0; k < 3; ++k) f[k] = (dword_of(vf[(3 * j + k) >> 4], ((3 * j + k) >> 2) & 3) >> (((3 * j + k) & 3) * 8)) & 255u;
            }
            shade<FRAME>(lds, s, f, CONTOUR && ((near >> j) & 1u) && s >= level, cc, o);
#pragma unroll
            for (int k = 0; k < 3; ++k) w[(3 * j + k) >> 2] |= o[k] << (((3 * j + k) & 3) * 8);
        }
        o4[3 * q] = make_uint4(w[0], w[1], w[2], w[3]);
        o4[3 * q + 1] = make_uint4(w[4], w[5], w[6], w[7]);
        o4[3 * q + 2] = make_uint4(w[8], w[9], w[10], w[11]);
    }
    // the head and the tail, pixel by pixel
    const int body = cut.words * 16, rest = len - body;
    for (int e = li; e < rest; e += nl) {
        const int i = e < cut.head ? e : e + body;
        const unsigned s = ps[i];
        unsigned f[3] = {0u, 0u, 0u}, o[3];
        if (FRAME) { f[0] = pf[3 * i]; f[1] = pf[3 * i + 1]; f[2] = pf[3 * i + 2]; }
        const bool near = CONTOUR && ((crow[(cb + i) >> 5] >> ((cb + i) & 31)) & 1u);
        shade<FRAME>(lds, s, f, near && s >= level, cc, o);
        po[3 * i] = (unsigned char)o[0]; po[3 * i + 1] = (unsigned char)o[1]; po[3 * i + 2] = (unsigned char)o[2];
    }
}

template <bool FRAME>
__device__ __forceinline__ void stage_table(unsigned* lds, const unsigned* table, int tid) {
    for (int v = tid; v < 256; v += TPB) {
        const unsigned e = table[v];
        if (FRAME) {
            const unsigned o = e >> 24;
            lds[2 * v] = ((e & 255u) * o + 127u) | ((((e >> 8) & 255u) * o + 127u) << 16);
            lds[2 * v + 1] = (((e >> 16) & 255u) * o + 127u) | ((255u - o) << 16);
        } else {
            lds[v] = e;
        }
    }
}

template <bool FRAME, bool CONTOUR>
__global__ __launch_bounds__(TPB) void render_kernel(RenderArgs a) {
    __shared__ unsigned lds[FRAME ? 512 : 256];
    __shared__ unsigned below[CONTOUR ? HALO_ROWS * ROW_WORDS : 1];      // s < L, one bit a pixel of the tile and its halo; then the window's OR
    __shared__ unsigned wide[CONTOUR ? HALO_ROWS * ROW_WORDS : 1];       // OR over |dx| <= t
    const int tid = threadIdx.x, m = blockIdx.y;
    const unsigned blk = blockIdx.x + blockIdx.z * gridDim.x;      // the grid folds blocks past RENDER_GRID_X into z
    if (blk >= (unsigned)a.blocks) return;
    const int n_pix = a.H * a.W;
    const unsigned char* ms = a.sal + (size_t)m * n_pix;
    const unsigned char* mf = FRAME ? a.frames + (size_t)m * n_pix * 3 : ms;
    unsigned char* mo = a.out + (size_t)m * n_pix * 3;
    stage_table<FRAME>(lds, a.table, tid);
    if (!CONTOUR) {
        __syncthreads();
        const int i0 = (int)min((long long)blk * a.chunk, (long long)n_pix), len = min(a.chunk, n_pix - i0);
        render_run<FRAME, false>(lds, ms + i0, mf + 3 * (size_t)i0, mo + 3 * (size_t)i0, len, tid, TPB, 0u, 0u, nullptr, 0);
        return;
    }
    const int t = a.thick, L = a.level;
    const int tiles_x = (a.W + TC - 1) / TC;
    const int y0 = (int)(blk / tiles_x) * TR, x0 = (int)(blk % tiles_x) * TC;
    const int halo_rows = TR + 2 * t;
    if (tid < HALO_ROWS * ROW_WORDS) below[tid] = 0u;
    __syncthreads();
    // halo column hc of the LDS rows is map column x0 - t + hc; half a wave takes one halo row
    for (int r = tid >> 5; r < halo_rows; r += TPB / 32) {
        const int gy = y0 - t + r, li = tid & 31;
        if (gy < 0 || gy >= a.H) continue;
        const int gx0 = max(0, x0 - t), gx1 = min(a.W, x0 + TC + t), len = gx1 - gx0, hc0 = gx0 - (x0 - t);
        const unsigned char* ps = ms + (size_t)gy * a.W + gx0;
        const int head = min(len, (int)((16 - ((uintptr_t)ps & 15)) & 15)), words = (len - head) >> 4, rest = len - words * 16;
        unsigned* row = below + r * ROW_WORDS;
        if (li < words) {
            const uint4 vs = *reinterpret_cast<const uint4*>(ps + head + 16 * li);
            unsigned mask = 0u;
#pragma unroll
            for (int j = 0; j < 16; ++j) mask |= (byte_of(vs, j) < (unsigned)L ? 1u : 0u) << j;
            const int p = hc0 + head + 16 * li;
            if (mask) {
                atomicOr(&row[p >> 5], mask << (p & 31));
                if ((p & 31) > 16) atomicOr(&row[(p >> 5) + 1], mask >> (32 - (p & 31)));
            }
        }
        if (li < rest) {
            const int i = li < head ? li : li + words * 16;
            if (ps[i] < (unsigned)L) atomicOr(&row[(hc0 + i) >> 5], 1u << ((hc0 + i) & 31));
        }
    }
    __syncthreads();
    if (tid < halo_rows * ROW_WORDS) {
        const int k = tid % ROW_WORDS;
        const unsigned cur = below[tid], prev = k > 0 ? below[tid - 1] : 0u, next = k < ROW_WORDS - 1 ? below[tid + 1] : 0u;
        unsigned v = cur;
        for (int d = 1; d <= t; ++d) v |= (cur >> d) | (next << (32 - d)) | (cur << d) | (prev >> (32 - d));
        wide[tid] = v;
    }
    __syncthreads();
    if (tid < TR * ROW_WORDS) {      // row r of the tile is halo row r + t: the rows r .. r + 2 t
        unsigned v = 0u;
        for (int j = 0; j <= 2 * t; ++j) v |= wide[tid + j * ROW_WORDS];
        below[tid] = v;
    }
    __syncthreads();
    const int r = tid >> 4, gy = y0 + r;
    if (gy >= a.H) return;
    const int len = min(TC, a.W - x0);
    const size_t at = (size_t)gy * a.W + x0;
    const unsigned cc = (unsigned)a.contour_bgr[0] | ((unsigned)a.contour_bgr[1] << 8) | ((unsigned)a.contour_bgr[2] << 16);
    render_run<FRAME, true>(lds, ms + at, mf + 3 * at, mo + 3 * at, len, tid & 15, 16, (unsigned)L, cc, below + r * ROW_WORDS, t);
}

bool args_ok(const RenderArgs& a) {
    if (!a.sal || !a.out || !a.table || a.n < 1 || a.n > 65535 || a.H < 1 || a.W < 1 || (long long)a.H * a.W > P3D_RENDER_MAX_PIXELS) return false;
    if (a.level < 0 || a.level > 255) return false;
    if (a.level > 0 && (a.thick < 1 || a.thick > MAXT)) return false;
    const RenderPlan p = p3d_render_plan(a.H, a.W, a.level > 0 ? a.thick : 0);
    return a.rows == p.rows && a.cols == p.cols && a.chunk == p.chunk && a.blocks == p.blocks;
}

}  // namespace

RenderPlan p3d_render_plan(int H, int W, int thick) {
    RenderPlan p;
    const long long n_pix = (long long)H * W;
    if (thick > 0) {
        p.rows = TR; p.cols = TC; p.chunk = TR * TC;
        p.blocks = (long long)((H + TR - 1) / TR) * ((W + TC - 1) / TC);
    } else {
        p.rows = 0; p.cols = 0; p.chunk = RENDER_CHUNK;
        p.blocks = (n_pix + RENDER_CHUNK - 1) / RENDER_CHUNK;
    }
    return p;
}

hipError_t p3d_render_launch(const RenderArgs& a, hipStream_t s) {
    if (!args_ok(a) || a.blocks > INT32_MAX) return hipErrorInvalidValue;
    // at most RENDER_GRID_X blocks in x, the rest folded into z: a grid dimension holds fewer than 2^32 threads, and a map one
    // pixel wide has up to 2^24 tiles
    const unsigned gx = (unsigned)std::min<long long>(a.blocks, RENDER_GRID_X), gz = (unsigned)((a.blocks + gx - 1) / gx);
    const dim3 grid(gx, (unsigned)a.n, gz), block(TPB);
    if (a.level > 0) {
        if (a.frames) hipLaunchKernelGGL((render_kernel<true, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((render_kernel<false, true>), grid, block, 0, s, a);
    } else {
        if (a.frames) hipLaunchKernelGGL((render_kernel<true, false>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((render_kernel<false, false>), grid, block, 0, s, a);
    }
    return hipGetLastError();
}
