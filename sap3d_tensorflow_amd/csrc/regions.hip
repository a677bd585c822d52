// Connected regions of 8-bit saliency maps (p3d_video_regions, p3d_regions_u8; RegionsArgs in p3d_kernels.h, the law in
// include/p3d_hip.h, "Salient regions of 8-bit maps"): per map the components of the gated pixels, their statistics, the K heaviest
// as records and as a label map, and identities linked from frame to frame by overlap.  Integer arithmetic throughout: every
// cross-block combination is an integer atomic (add / min / max), which commutes, so no order can show.
//
// p3d_regions_plan's maps_per_chunk maps at a time; per chunk, each step a launch of its own -- a launch boundary is the fence that
// makes one step's stores visible to the next on every XCD, and no loop anywhere waits on another block:
//  * regions_label: grid (tiles, maps), a block a tile of 32 x 64 pixels.  The tile's bytes come in by 16-byte loads in the words of
//    each row's own alignment (bytes of a word outside the row are read one by one, and only inside the row).  A wave takes a row, a
//    lane a column: a ballot gives every pixel the start of its row run, so a run is one label from the outset and a serpentine does
//    not take a sweep per pixel.  Runs of neighbouring rows are united in a union-find in LDS (atomicMin on the larger root); the
//    local roots go out as global linear indices -- for foreground pixels only: the background is known from the bytes and its
//    entries of the parent array are neither written nor read -- and every local root clears its slot of the tables (a global root
//    is the smallest index of its component, hence also of its part of the tile: it is among them).  The map's two counters are
//    zeroed here.
//  * regions_seams: grid (tiles, maps).  The pixels of a tile's top row and left column unite with their neighbours across the
//    border in the global parent array.  Blocks on different XCDs share that array inside this launch: every access to it here is an
//    agent-scope atomic (__hip_atomic_load, atomicMin).
//  * regions_stats: grid (tiles, maps).  The first lane of a row run walks to its ROOT (plain loads: the launch before has ended),
//    the run's lanes fold area, mass, sum of s * x and the peak by a segmented scan over shuffles, and the run's last lane issues one
//    atomic per field into the root's slot: 32-bit adds for AREA and MASS, 64-bit adds for SY and SX, min / max for the box, and one
//    max of (byte << 23 | ~index) for PEAK and its position.  Every foreground pixel is rewritten with its ROOT; the pixels that are
//    their own ROOT are counted per block in LDS and take their places in the map's list of components with one atomic a block (one
//    a pixel made a checkerboard's half a million components queue at one address).
//  * regions_select: a block a map.  A component's key is (MASS << 32 | ~ROOT) when AREA >= min_area, else 0: keys are distinct (ROOT
//    is) and the largest is the first in the order of SELECTION.  The keys replace the list in place; every thread holds the largest
//    of its share; K rounds take the block's largest, and only the thread that owned it looks for its next.  Then a thread a
//    record, the root's rank into the rank table, the counts, and the map's overlap table zeroed for the link.
//  * regions_remap (label maps asked for, or link): root -> rank, written as 16-byte words of bytes where the destination allows.
//  * regions_overlap + regions_link (link): O [K][K] of every frame pair counted in LDS from the two label maps (a word of 16
//    background bytes is skipped whole), then one block: a wave a frame finds every region's PREV, OVERLAP and whether it is its
//    PREV's heir, and the first wave walks the chunk's frames in order and hands out the IDs.  The counter and
//    the last frame's IDs wait in `state` for the next chunk; without the caller's label maps they live in a ring of
//    maps_per_chunk + 1 slots, frame f in slot (f + 1) mod that, so the chunk's frames never overwrite the one before them.
#include "p3d_kernels.h"
#include "../../include/p3d_hip.h"
#include <algorithm>

static_assert(P3D_REGIONS_K == P3D_REGIONS_MAX && P3D_REGIONS_NFIELDS == P3D_REGION_FIELDS, "p3d_kernels.h names the header's numbers");

namespace {

constexpr int TPB = 256, WAVE = 64, WAVES = TPB / WAVE, TH = REGIONS_TILE_H, TW = REGIONS_TILE_W, TPIX = TH * TW;
constexpr int ROW_WORDS = TW / 16 + 1;                  // a row of TW bytes at any alignment lies in at most this many aligned words
constexpr int SEL_TPB = 1024, K = P3D_REGIONS_K, NF = P3D_REGIONS_NFIELDS;
constexpr int LINK_TPB = WAVE * P3D_REGIONS_CHUNK;
constexpr int OVL_BLOCKS = 64;                          // blocks that share the pixels of one frame pair
constexpr unsigned ALL = 0xffffffffu, BIG = 0x7fffffffu, IDX = (1u << 23) - 1u;
static_assert(TW == WAVE, "a lane a column");
static_assert(LINK_TPB <= 1024, "the link takes a wave a frame of a chunk in one block");
static_assert(P3D_REGIONS_MAX_PIXELS - 1 == (int)IDX, "a peak key is a byte above a 23-bit index");
enum { T_AREA = 0, T_MASS = 1, T_Y0 = 2, T_X0 = 3, T_Y1 = 4, T_X1 = 5, T_PEAK = 6, T32 = P3D_REGIONS_TAB32, T_SY = 0, T_SX = 1, T64 = P3D_REGIONS_TAB64 };

__device__ __forceinline__ unsigned dword_of(const uint4& v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }
__device__ __forceinline__ unsigned byte_of(const uint4& v, int j) { return (dword_of(v, j >> 2) >> ((j & 3) * 8)) & 255u; }
__device__ __forceinline__ long long slot_of(unsigned root, int W) { const unsigned y = root / (unsigned)W; return (long long)y * ((W + 1) >> 1) + ((root - y * (unsigned)W) >> 1); }

// The bytes of the tile at (y0, x0) of one map into val [TH][TW]; outside the map 0, which no gate passes
__device__ void load_tile(const unsigned char* map, int H, int W, int y0, int x0, unsigned char* val) {
    const int th = min(TH, H - y0), tw = min(TW, W - x0);
    for (int i = threadIdx.x; i < TPIX / 4; i += TPB) reinterpret_cast<unsigned*>(val)[i] = 0u;
    __syncthreads();
    for (int t = threadIdx.x; t < th * ROW_WORDS; t += TPB) {
        const int r = t / ROW_WORDS, q = t - r * ROW_WORDS;
        const unsigned char* ps = map + (size_t)(y0 + r) * W + x0;
        const int off = (int)((uintptr_t)ps & 15), words = (off + tw + 15) >> 4;
        if (q >= words) continue;
        const unsigned char* pw = ps - off + q * 16;
        const int xs = q * 16 - off;
        unsigned char* o = val + r * TW;
        if (xs >= 0 && xs + 16 <= tw) {
            const uint4 v = *reinterpret_cast<const uint4*>(pw);
#pragma unroll
            for (int j = 0; j < 16; ++j) o[xs + j] = (unsigned char)byte_of(v, j);
        } else {
            for (int j = 0; j < 16; ++j)
                if (xs + j >= 0 && xs + j < tw) o[xs + j] = pw[j];
        }
    }
    __syncthreads();
}

// the start of lane's row run: the lane after the highest background lane below it
__device__ __forceinline__ int run_start(unsigned long long fg, int lane) {
    const unsigned long long below = ~fg & ((1ull << lane) - 1ull);
    return below ? 64 - __clzll((long long)below) : 0;
}
// the last lane of lane's row run
__device__ __forceinline__ int run_end(unsigned long long fg, int lane) {
    const unsigned long long above = lane == 63 ? 0ull : (~fg >> (lane + 1)) << (lane + 1);
    return above ? __ffsll((long long)above) - 2 : 63;
}

__device__ __forceinline__ int lds_load(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int lds_find(int* par, int x) {
    int p;
    while ((p = lds_load(par + x)) != x) x = p;             // ends: a pixel that is no root points to a smaller index, so x falls strictly
    return x;
}
__device__ __forceinline__ void lds_union(int* par, int a, int b) {
    for (;;) {                                              // ends: a turn either returns or lowers a (old < a), and indices are bounded below
        a = lds_find(par, a); b = lds_find(par, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&par[a], b);
        if (old == a) return;
        a = old;
    }
}
__device__ __forceinline__ unsigned agent_load(unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned agent_find(unsigned* par, unsigned x) {
    unsigned p;
    while ((p = agent_load(par + x)) != x) x = p;           // ends: as lds_find; a concurrent atomicMin only lowers what a pixel points to
    return x;
}
__device__ __forceinline__ void agent_union(unsigned* par, unsigned a, unsigned b) {
    for (;;) {                                              // ends: as lds_union
        a = agent_find(par, a); b = agent_find(par, b);
        if (a == b) return;
        if (a < b) { const unsigned t = a; a = b; b = t; }
        const unsigned old = atomicMin(&par[a], b);
        if (old == a) return;
        a = old;
    }
}

__global__ __launch_bounds__(TPB) void regions_label(RegionsArgs a, int m0) {
    __shared__ __attribute__((aligned(16))) unsigned char val[TPIX];
    __shared__ int par[TPIX];
    const int tile = blockIdx.x, m = blockIdx.y, ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x, y0 = ty * TH, x0 = tx * TW;
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    if (tile == 0 && threadIdx.x < 2) a.cnt[2 * m + threadIdx.x] = 0u;
    load_tile(a.sal + (size_t)(m0 + m) * a.H * a.W, a.H, a.W, y0, x0, val);
    const unsigned g = (unsigned)a.gate;
    for (int r = wave; r < TH; r += WAVES) {
        const bool fg = val[r * TW + lane] >= g;
        const unsigned long long mask = __ballot(fg);
        par[r * TW + lane] = fg ? r * TW + run_start(mask, lane) : -1;
    }
    __syncthreads();
    for (int y = 1 + wave; y < TH; y += WAVES) {            // (row 0 has nothing above it)
        const int p = y * TW + lane;
        if (val[p] < g) continue;
        const bool up = val[p - TW] >= g, left = lane > 0 && val[p - 1] >= g, upleft = lane > 0 && val[p - TW - 1] >= g;
        // the pair of runs (this row's, the row's above) is united once, at the leftmost column they share
        if (up && !(left && upleft)) lds_union(par, p, p - TW);
        if (a.conn == 8 && !up) {                           // (with `up` set, the diagonals lie in its run)
            if (upleft) lds_union(par, p, p - TW - 1);
            if (lane + 1 < TW && val[p - TW + 1] >= g) lds_union(par, p, p - TW + 1);
        }
    }
    __syncthreads();
    const long long S = a.slots;
    unsigned* t32 = a.tab32 + (size_t)m * T32 * S;
    unsigned long long* t64 = a.tab64 + (size_t)m * T64 * S;
    for (int r = wave; r < TH; r += WAVES) {
        const int p = r * TW + lane;
        if (val[p] < g) continue;                           // (pixels outside the map hold 0)
        const int root = lds_find(par, p);
        const unsigned out = (unsigned)((y0 + root / TW) * a.W + x0 + (root & (TW - 1)));
        if (root == p) {
            const long long sl = slot_of(out, a.W);
            t32[T_AREA * S + sl] = 0u; t32[T_MASS * S + sl] = 0u; t32[T_Y0 * S + sl] = BIG; t32[T_X0 * S + sl] = BIG;
            t32[T_Y1 * S + sl] = 0u; t32[T_X1 * S + sl] = 0u; t32[T_PEAK * S + sl] = 0u;
            t64[T_SY * S + sl] = 0ull; t64[T_SX * S + sl] = 0ull;
            a.rank[(size_t)m * S + sl] = 255;
        }
        a.parent[(size_t)m * a.H * a.W + (size_t)(y0 + r) * a.W + x0 + lane] = out;
    }
}

__global__ __launch_bounds__(TPB) void regions_seams(RegionsArgs a, int m0) {
    const int tile = blockIdx.x, m = blockIdx.y, ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x, y0 = ty * TH, x0 = tx * TW;
    unsigned* par = a.parent + (size_t)m * a.H * a.W;
    const unsigned char* sal = a.sal + (size_t)(m0 + m) * a.H * a.W;
    const unsigned g = (unsigned)a.gate;
    const int t = threadIdx.x, W = a.W, H = a.H;
    const bool diag = a.conn == 8;
    if (t < TW) {                                           // the top row against the row above the tile
        const int y = y0, x = x0 + t;
        if (y == 0 || x >= W) return;
        const unsigned p = (unsigned)(y * W + x);
        if (sal[p] < g) return;
        if (sal[p - W] >= g) agent_union(par, p, p - W);
        if (diag && x > 0 && sal[p - W - 1] >= g) agent_union(par, p, p - W - 1);
        if (diag && x + 1 < W && sal[p - W + 1] >= g) agent_union(par, p, p - W + 1);
    } else if (t < TW + TH) {                               // the left column against the column left of the tile
        const int y = y0 + t - TW, x = x0;
        if (x == 0 || y >= H) return;
        const unsigned p = (unsigned)(y * W + x);
        if (sal[p] < g) return;
        if (sal[p - 1] >= g) agent_union(par, p, p - 1);
        if (diag && y > 0 && sal[p - W - 1] >= g) agent_union(par, p, p - W - 1);
        if (diag && y + 1 < H && sal[p + W - 1] >= g) agent_union(par, p, p + W - 1);
    }
}

__global__ __launch_bounds__(TPB) void regions_stats(RegionsArgs a, int m0) {
    __shared__ __attribute__((aligned(16))) unsigned char val[TPIX];
    __shared__ unsigned long long rmask[TH];                // per row: the lanes that are their component's ROOT
    __shared__ unsigned rbase[TH], cnt[1], gbase;
    const int tile = blockIdx.x, m = blockIdx.y, ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x, y0 = ty * TH, x0 = tx * TW;
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    if (threadIdx.x < TH) rmask[threadIdx.x] = 0ull;
    if (threadIdx.x == 0) cnt[0] = 0u;
    load_tile(a.sal + (size_t)(m0 + m) * a.H * a.W, a.H, a.W, y0, x0, val);
    const unsigned g = (unsigned)a.gate;
    const long long S = a.slots;
    unsigned* par = a.parent + (size_t)m * a.H * a.W;
    unsigned* t32 = a.tab32 + (size_t)m * T32 * S;
    unsigned long long* t64 = a.tab64 + (size_t)m * T64 * S;
    for (int r = wave; r < TH; r += WAVES) {
        const int y = y0 + r;
        if (y >= a.H) break;                                // (the whole wave)
        const unsigned v = val[r * TW + lane];
        const bool fg = v >= g;
        const unsigned long long mask = __ballot(fg);
        if (!mask) continue;
        const int st = run_start(mask, lane), en = run_end(mask, lane);
        const unsigned p = (unsigned)(y * a.W + x0 + lane);
        unsigned root = ALL;
        if (fg && lane == st) {
            unsigned x = p, q;
            while ((q = par[x]) != x) x = q;                // ends: as lds_find.  A pixel another block has rewritten by now points to its ROOT
            root = x;
        }
        root = __shfl(root, fg ? st : lane);
        const unsigned long long roots = __ballot(fg && root == p);
        if (roots && lane == 0) { rbase[r] = atomicAdd(&cnt[0], (unsigned)__popcll(roots)); rmask[r] = roots; }
        // segmented inclusive scans over the run: the mass, the sum of v * (lane - st), the peak key (byte, then the lower lane)
        unsigned mass = fg ? v : 0u, mom = fg ? v * (unsigned)(lane - st) : 0u, peak = fg ? (v << 8) | (unsigned)(63 - lane) : 0u;
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            const unsigned tm = __shfl_up(mass, d), to = __shfl_up(mom, d), tp = __shfl_up(peak, d);
            if (fg && lane - d >= st) { mass += tm; mom += to; peak = max(peak, tp); }
        }
        if (fg) par[p] = root;
        if (fg && lane == en) {
            const long long sl = slot_of(root, a.W);
            const unsigned area = (unsigned)(en - st + 1), xs = (unsigned)(x0 + st), xe = (unsigned)(x0 + en);
            const unsigned long long sy = (unsigned long long)mass * (unsigned)y, sx = (unsigned long long)mass * xs + mom;
            const unsigned pv = peak >> 8, px = (unsigned)x0 + 63u - (peak & 255u);
            const unsigned pk = (pv << 23) | (IDX - ((unsigned)y * (unsigned)a.W + px));
            __hip_atomic_fetch_add(&t32[T_AREA * S + sl], area, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(&t32[T_MASS * S + sl], mass, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(&t64[T_SY * S + sl], sy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(&t64[T_SX * S + sl], sx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            atomicMin(&t32[T_Y0 * S + sl], (unsigned)y); atomicMax(&t32[T_Y1 * S + sl], (unsigned)y);
            atomicMin(&t32[T_X0 * S + sl], xs); atomicMax(&t32[T_X1 * S + sl], xe);
            atomicMax(&t32[T_PEAK * S + sl], pk);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned total = cnt[0];
        gbase = total ? __hip_atomic_fetch_add(&a.cnt[2 * m], total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    }
    __syncthreads();
    for (int r = wave; r < TH; r += WAVES) {
        const unsigned long long roots = rmask[r];
        if ((roots >> lane) & 1ull)
            a.keys[(size_t)m * S + gbase + rbase[r] + (unsigned)__popcll(roots & ((1ull << lane) - 1ull))] = (unsigned)((y0 + r) * a.W + x0 + lane);
    }
}

__global__ __launch_bounds__(SEL_TPB) void regions_select(RegionsArgs a, int m0) {
    __shared__ unsigned long long wbest[SEL_TPB / WAVE], sel[K];
    __shared__ unsigned long long top;
    __shared__ unsigned wbig[SEL_TPB / WAVE], sbig;
    const int m = blockIdx.x, f = m0 + m, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
    const long long S = a.slots;
    const unsigned nc = a.cnt[2 * m];
    const unsigned* t32 = a.tab32 + (size_t)m * T32 * S;
    const unsigned long long* t64 = a.tab64 + (size_t)m * T64 * S;
    unsigned long long* keys = a.keys + (size_t)m * S;
    if (a.link)
        for (int i = tid; i < K * K; i += SEL_TPB) a.ovl[(size_t)m * K * K + i] = 0u;
    // the list's roots become keys, in place; every thread keeps the largest of its share
    unsigned long long best = 0ull;
    unsigned big = 0u;
    for (unsigned i = tid; i < nc; i += SEL_TPB) {
        const unsigned root = (unsigned)keys[i];
        const long long sl = slot_of(root, a.W);
        const bool ok = t32[T_AREA * S + sl] >= (unsigned)a.min_area;
        const unsigned long long k = ok ? ((unsigned long long)t32[T_MASS * S + sl] << 32) | (ALL - root) : 0ull;
        keys[i] = k;
        best = max(best, k);
        big += ok ? 1u : 0u;
    }
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) big += __shfl_xor(big, o);
    if (lane == 0) wbig[wave] = big;
    __syncthreads();
    if (tid == 0) {
        unsigned t = 0u;
        for (int k = 0; k < SEL_TPB / WAVE; ++k) t += wbig[k];
        sbig = t;
    }
    __syncthreads();
    const unsigned nbig = sbig;
    const int kept = (int)min(nbig, (unsigned)a.K);
    for (int r = 0; r < kept; ++r) {
        unsigned long long b = best;
#pragma unroll
        for (int o = WAVE / 2; o > 0; o >>= 1) b = max(b, (unsigned long long)__shfl_xor(b, o));
        if (lane == 0) wbest[wave] = b;
        __syncthreads();
        if (tid == 0) {
            unsigned long long t = wbest[0];
            for (int k = 1; k < SEL_TPB / WAVE; ++k) t = max(t, wbest[k]);
            top = t; sel[r] = t;
        }
        __syncthreads();
        const unsigned long long t = top;
        if (best == t) {                                    // keys are distinct: one thread, which looks for its next below t
            best = 0ull;
            for (unsigned i = tid; i < nc; i += SEL_TPB) { const unsigned long long k = keys[i]; if (k < t) best = max(best, k); }
        }
    }
    __syncthreads();
    if (tid == 0 && a.counts) { a.counts[3 * (size_t)f] = (int)nc; a.counts[3 * (size_t)f + 1] = (int)nbig; a.counts[3 * (size_t)f + 2] = kept; }
    if (tid == 0) a.cnt[2 * m + 1] = (unsigned)kept;        // (the link reads the kept count here)
    if (tid >= a.K) return;
    int32_t* o = a.regions + ((size_t)f * a.K + tid) * NF;
    if (tid >= kept) {
        for (int k = 0; k < NF; ++k) o[k] = -1;
        return;
    }
    const unsigned root = ALL - (unsigned)(sel[tid] & 0xffffffffull);
    const long long sl = slot_of(root, a.W);
    const unsigned long long mass = t32[T_MASS * S + sl];
    const unsigned pk = t32[T_PEAK * S + sl], pidx = IDX - (pk & IDX);
    o[P3D_REGION_ROOT] = (int)root; o[P3D_REGION_AREA] = (int)t32[T_AREA * S + sl]; o[P3D_REGION_MASS] = (int)mass;
    o[P3D_REGION_Y0] = (int)t32[T_Y0 * S + sl]; o[P3D_REGION_X0] = (int)t32[T_X0 * S + sl];
    o[P3D_REGION_Y1] = (int)t32[T_Y1 * S + sl]; o[P3D_REGION_X1] = (int)t32[T_X1 * S + sl];
    o[P3D_REGION_PEAK] = (int)(pk >> 23); o[P3D_REGION_PEAK_Y] = (int)(pidx / (unsigned)a.W); o[P3D_REGION_PEAK_X] = (int)(pidx % (unsigned)a.W);
    o[P3D_REGION_CY] = (int)((2ull * t64[T_SY * S + sl] + mass) / (2ull * mass));
    o[P3D_REGION_CX] = (int)((2ull * t64[T_SX * S + sl] + mass) / (2ull * mass));
    o[P3D_REGION_ID] = -1; o[P3D_REGION_PREV] = -1; o[P3D_REGION_OVERLAP] = 0;
    a.rank[(size_t)m * S + sl] = (unsigned char)tid;
}

// where frame f's label map lies: in the caller's [n][H W], or in the ring's slot (f + 1) mod (maps_per_chunk + 1)
__device__ __forceinline__ size_t lab_at(const RegionsArgs& a, int f) {
    return (size_t)(a.lab_full ? f : (f + 1) % (a.maps_per_chunk + 1)) * (size_t)a.H * (size_t)a.W;
}

__global__ __launch_bounds__(TPB) void regions_remap(RegionsArgs a, int m0) {
    const int m = blockIdx.y, HW = a.H * a.W;
    unsigned char* lab = a.lab + lab_at(a, m0 + m);
    const unsigned char* sal = a.sal + (size_t)(m0 + m) * HW;
    const unsigned* par = a.parent + (size_t)m * HW;
    const unsigned char* rank = a.rank + (size_t)m * a.slots;
    const unsigned g = (unsigned)a.gate;
    const int off = (int)((uintptr_t)lab & 15), words = (off + HW + 15) >> 4;
    const int q = blockIdx.x * TPB + threadIdx.x;
    if (q >= words) return;
    const int i0 = q * 16 - off;
    if (i0 >= 0 && i0 + 16 <= HW) {
        unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const unsigned b = sal[i0 + j] >= g ? rank[slot_of(par[i0 + j], a.W)] : 255u;
            w[j >> 2] |= b << ((j & 3) * 8);
        }
        *reinterpret_cast<uint4*>(lab + i0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        for (int j = 0; j < 16; ++j) {
            const int i = i0 + j;
            if (i < 0 || i >= HW) continue;
            lab[i] = sal[i] >= g ? rank[slot_of(par[i], a.W)] : (unsigned char)255;
        }
    }
}

// frame 0 of the call and the first frame of every shot
__device__ __forceinline__ bool is_start(const RegionsArgs& a, int f) {
    if (f == 0) return true;
    if (!a.starts) return false;
    int lo = 0, hi = a.n_shots - 1;                         // the last shot that starts at or before f
    while (lo < hi) {                                       // ends: the interval shrinks every turn
        const int mid = (lo + hi + 1) >> 1;
        if (a.starts[mid] <= f) lo = mid; else hi = mid - 1;
    }
    return a.starts[lo] == f;
}

__global__ __launch_bounds__(TPB) void regions_overlap(RegionsArgs a, int m0) {
    __shared__ unsigned cnt[K * K];
    const int m = blockIdx.y, f = m0 + m, HW = a.H * a.W;
    if (is_start(a, f)) return;                             // (the whole block)
    for (int i = threadIdx.x; i < K * K; i += TPB) cnt[i] = 0u;
    __syncthreads();
    const unsigned char* cur = a.lab + lab_at(a, f);
    const unsigned char* prev = a.lab + lab_at(a, f - 1);
    const int off = (int)((uintptr_t)cur & 15), words = (off + HW + 15) >> 4;
    for (int q = blockIdx.x * TPB + threadIdx.x; q < words; q += OVL_BLOCKS * TPB) {
        const int i0 = q * 16 - off;
        if (i0 >= 0 && i0 + 16 <= HW) {
            const uint4 v = *reinterpret_cast<const uint4*>(cur + i0);
            if ((v.x & v.y & v.z & v.w) == ALL) continue;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const unsigned c = byte_of(v, j);
                if (c == 255u) continue;
                const unsigned p = prev[i0 + j];
                if (p != 255u) atomicAdd(&cnt[c * K + p], 1u);
            }
        } else {
            for (int j = 0; j < 16; ++j) {
                const int i = i0 + j;
                if (i < 0 || i >= HW) continue;
                const unsigned c = cur[i], p = prev[i];
                if (c != 255u && p != 255u) atomicAdd(&cnt[c * K + p], 1u);
            }
        }
    }
    __syncthreads();
    unsigned* out = a.ovl + (size_t)m * K * K;
    for (int i = threadIdx.x; i < K * K; i += TPB) {
        const unsigned v = cnt[i];
        if (v) __hip_atomic_fetch_add(&out[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// A wave a frame of the chunk, a lane a column of O: PREV and OVERLAP of region j are a wave maximum over row j, read coalesced, of
// (count << 6 | 63 - i), so that the smaller i wins among equals.  HEIR needs no second read: O[j][PREV(j)] is OVERLAP(j), and j is
// its PREV's heir unless another region with the same PREV overlaps it more, or as much with a smaller rank.  Then the first wave
// alone walks the frames in order and hands out the IDs; the last frame's IDs travel from frame to frame in a register a lane.
__global__ __launch_bounds__(LINK_TPB) void regions_link(RegionsArgs a, int m0, int maps) {
    __shared__ int sprev[P3D_REGIONS_CHUNK][K], sfrom[P3D_REGIONS_CHUNK][K], skept[P3D_REGIONS_CHUNK];
    __shared__ unsigned sov[P3D_REGIONS_CHUNK][K];
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x >> 6;
    int kept = 0, prev = -1;
    unsigned ov = 0u;
    if (w < maps) {
        const int f = m0 + w;
        kept = (int)a.cnt[2 * w + 1];
        const int pk = w ? (int)a.cnt[2 * (w - 1) + 1] : m0 ? a.state[1] : 0;
        const unsigned* O = a.ovl + (size_t)w * K * K;
        if (!is_start(a, f)) {
#pragma unroll 4
            for (int j = 0; j < kept; ++j) {
                const unsigned o = lane < pk ? O[j * K + lane] : 0u;      // (at most 2^23: the key fits a word)
                unsigned key = o ? (o << 6) | (unsigned)(63 - lane) : 0u;
#pragma unroll
                for (int d = WAVE / 2; d > 0; d >>= 1) key = max(key, (unsigned)__shfl_xor(key, d));
                if (lane == j && key) { prev = 63 - (int)(key & 63u); ov = key >> 6; }
            }
        }
        sprev[w][lane] = prev; sov[w][lane] = ov;
        if (lane == 0) skept[w] = kept;
    }
    __syncthreads();
    if (w < maps) {
        bool inherit = prev >= 0;
        for (int t = 0; t < kept && inherit; ++t)
            if (t != lane && sprev[w][t] == prev && (sov[w][t] > ov || (sov[w][t] == ov && t < lane))) inherit = false;
        sfrom[w][lane] = inherit ? prev : -1;
        if (lane < kept) {
            int32_t* o = a.regions + ((size_t)(m0 + w) * a.K + lane) * NF;
            o[P3D_REGION_PREV] = prev; o[P3D_REGION_OVERLAP] = (int)ov;
        }
    }
    __syncthreads();
    if (w != 0) return;
    int counter = m0 ? a.state[0] : 0, last = m0 ? a.state[2 + lane] : -1, pk = 0;
    for (int m = 0; m < maps; ++m) {
        const int from = sfrom[m][lane];
        pk = skept[m];
        const bool fresh = lane < pk && from < 0;
        const unsigned long long mask = __ballot(fresh);
        const int got = __shfl(last, from < 0 ? lane : from);
        const int id = from >= 0 ? got : counter + __popcll(mask & ((1ull << lane) - 1ull));
        counter += __popcll(mask);
        last = lane < pk ? id : -1;
        if (lane < pk) a.regions[((size_t)(m0 + m) * a.K + lane) * NF + P3D_REGION_ID] = id;
    }
    if (lane == 0) { a.state[0] = counter; a.state[1] = pk; }
    a.state[2 + lane] = last;
}

bool args_ok(const RegionsArgs& a) {
    if (!a.sal || !a.regions || !a.parent || !a.tab32 || !a.tab64 || !a.rank || !a.keys || !a.cnt) return false;
    if (a.n < 1 || a.n > 65535 || a.H < 1 || a.W < 1 || (long long)a.H * a.W > P3D_REGIONS_MAX_PIXELS) return false;
    if (a.gate < 1 || a.gate > 255 || (a.conn != 4 && a.conn != 8) || a.min_area < 1 || a.K < 1 || a.K > K) return false;
    if ((a.link != 0 && a.link != 1) || (a.lab_full != 0 && a.lab_full != 1)) return false;
    if ((a.link || a.lab_full) != (a.lab != nullptr)) return false;
    if (a.link && (!a.ovl || !a.state)) return false;
    if ((a.starts == nullptr) != (a.n_shots == 0) || a.n_shots < 0 || a.n_shots > a.n) return false;
    const RegionsPlan p = p3d_regions_plan(a.H, a.W, a.n, a.K, a.link, a.lab_full);
    return a.maps_per_chunk == p.maps_per_chunk && a.tiles_y == p.tiles_y && a.tiles_x == p.tiles_x && a.slots == p.slots;
}

}  // namespace

RegionsPlan p3d_regions_plan(int H, int W, int n, int /* max_regions: the tables are laid out for P3D_REGIONS_K */, int link, int lab_full) {
    RegionsPlan p;
    const long long hw = (long long)H * W;
    p.tile_h = TH; p.tile_w = TW;
    p.tiles_y = (H + TH - 1) / TH; p.tiles_x = (W + TW - 1) / TW;
    p.slots = (long long)H * ((W + 1) / 2);
    const long long per_map = 4 * hw + (4 * T32 + 8 * T64 + 1 + 8) * p.slots;
    p.maps_per_chunk = (int)std::max<long long>(1, std::min<long long>(std::min(n, P3D_REGIONS_CHUNK), P3D_REGIONS_SCRATCH_BYTES / per_map));
    const long long mpc = p.maps_per_chunk;
    p.parent_elems = mpc * hw; p.tab32_elems = mpc * T32 * p.slots; p.tab64_elems = mpc * T64 * p.slots; p.rank_elems = mpc * p.slots;
    p.key_elems = mpc * p.slots; p.cnt_elems = mpc * 2;
    p.ovl_elems = link ? mpc * K * K : 0; p.state_elems = link ? 2 + K : 0;
    p.lab_elems = lab_full ? (long long)n * hw : link ? (mpc + 1) * hw : 0;
    // every buffer from a 256-byte boundary
    const long long sizes[] = {p.parent_elems * 4, p.tab32_elems * 4, p.tab64_elems * 8, p.rank_elems, p.key_elems * 8, p.cnt_elems * 4,
                               p.ovl_elems * 4, p.state_elems * 4, p.lab_elems};
    for (long long b : sizes) p.scratch_bytes += (std::max<long long>(b, 1) + 255) & ~255LL;
    return p;
}

hipError_t p3d_regions_launch(const RegionsArgs& a, hipStream_t s) {
    if (!args_ok(a)) return hipErrorInvalidValue;
    const dim3 block(TPB);
    const size_t hw = (size_t)a.H * a.W;
    const unsigned tiles = (unsigned)(a.tiles_y * a.tiles_x);
    for (int m0 = 0; m0 < a.n; m0 += a.maps_per_chunk) {
        const unsigned maps = (unsigned)std::min(a.maps_per_chunk, a.n - m0);
        hipLaunchKernelGGL(regions_label, dim3(tiles, maps), block, 0, s, a, m0);
        if (tiles > 1) hipLaunchKernelGGL(regions_seams, dim3(tiles, maps), block, 0, s, a, m0);
        hipLaunchKernelGGL(regions_stats, dim3(tiles, maps), block, 0, s, a, m0);
        hipLaunchKernelGGL(regions_select, dim3(maps), dim3(SEL_TPB), 0, s, a, m0);
        if (a.lab) {
            const unsigned words = (unsigned)((hw + 15) / 16 + 1);
            hipLaunchKernelGGL(regions_remap, dim3((words + TPB - 1) / TPB, maps), block, 0, s, a, m0);
        }
        if (a.link) {
            hipLaunchKernelGGL(regions_overlap, dim3(OVL_BLOCKS, maps), block, 0, s, a, m0);
            hipLaunchKernelGGL(regions_link, dim3(1), dim3(LINK_TPB), 0, s, a, m0, (int)maps);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipGetLastError();
}
