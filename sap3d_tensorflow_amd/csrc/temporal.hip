// Temporal smoothing of a resident video's maps at read-out (p3d_set_video_temporal; the argument struct in p3d_kernels.h, the
// contract in include/p3d_hip.h).  The maps [F][hw] are filtered along the frame axis into [n][hw] of scratch; the store is only
// read.  Under MEAN a frame's input is sum / (float)count, divided as the frame is loaded: no finalised copy of the video exists.
//
//  * video_temporal_gauss_kernel<MEAN, V>: 256 lanes; blockIdx.x is a strip of 256 * V pixels, blockIdx.y a run of
//    frames_per_block consecutive output frames.  A lane owns V pixels and keeps their last 2r + 1 inputs in a ring in LDS,
//    ring[slot][lane] of 4 V bytes: consecutive lanes at consecutive addresses, so every access is conflict free, and a lane only
//    ever touches its own column, so the block needs no barrier.  V = 4 while the ring fits 64 KB (r <= 7): one float4 per lane
//    where hw is a multiple of 4 and both bases are 16-byte aligned, else pixels tid + k * 256, element by element; the LDS
//    accesses are 16 bytes either way.  V = 1 above that: a quarter of the ring per lane keeps four waves a block (and twelve a
//    CU) on the serial walk instead of one, which is worth more here than the wider loads.  Walking the run, every input frame
//    is loaded once (the next frame's load is in flight while the current output is summed), plus the r frames either side of
//    the run, GAUSS_PRELOAD loads in flight at a time.  The reflected taps at frames 0 and F - 1 are inside the ring already
//    (r <= F - 1).  The slots are tracked by increments: no division.
//  * video_temporal_ema_kernel<MEAN, V>: one lane per V pixels walks frames 0 .. first + n - 1 and stores from `first`.  The
//    recurrence is serial along f; the loads are not, and go out EMA_UNROLL frames at a time ahead of it.  Blocks of one wave
//    spread a small map over as many CUs as it has waves.  V = 4 only where hw is large enough to fill the chip with float4 lanes.
//  * Under a shot table (p3d_video_set_shots) the two *_shots_kernel twins run the same bodies from a run table (f0, f1, lo, hi) in
//    scratch (p3d_video_temporal_runs): the reflections bounce at the ends lo and hi of the run's shot, periodically, so a shot
//    shorter than the radius is legal; the moving average restarts at every shot.  Without a table the launches are the old ones.
// No atomics, no cross-block state; every operation rounds on its own.
#include "p3d_kernels.h"
#include <algorithm>
#include <vector>

#pragma clang fp contract(off)

namespace {

constexpr int EMA_TPB = 64, EMA_UNROLL = 16;
constexpr long long EMA_VEC_MIN_HW = 1ll << 18;      // float4 lanes from here on: at least one wave per SIMD of the chip
constexpr int GAUSS_TPB = 256, GAUSS_PRELOAD = 8;
constexpr int GAUSS_LDS_MAX = 65536;                 // no opt-in needed
constexpr int GAUSS_TARGET_BLOCKS = 1024, GAUSS_MIN_RUN = 8;

__device__ __forceinline__ bool aligned16(const void* a, const void* b) {
    return (((unsigned long long)a | (unsigned long long)b) & 15ull) == 0;
}

// the V pixels of a lane
template <int V> struct Pix;
template <> struct Pix<1> {
    float x;
    __device__ __forceinline__ static Pix zero() { return {0.f}; }
    __device__ __forceinline__ static Pix ld(const float* p) { return {*p}; }
    __device__ __forceinline__ void st(float* p) const { *p = x; }
    __device__ __forceinline__ void div(float d) { x = __fdiv_rn(x, d); }
    __device__ __forceinline__ static Pix scaled(float w, const Pix& c) { return {w * c.x}; }
    __device__ __forceinline__ void tap(float w, const Pix& u, const Pix& v) { x = x + w * (u.x + v.x); }      // PASS
    __device__ __forceinline__ void step(float al, float b, const Pix& v) { x = al * x + b * v.x; }             // EMA
};
template <> struct Pix<4> {
    float4 q;
    __device__ __forceinline__ static Pix zero() { return {make_float4(0.f, 0.f, 0.f, 0.f)}; }
    __device__ __forceinline__ static Pix ld(const float* p) { return {*reinterpret_cast<const float4*>(p)}; }
    __device__ __forceinline__ void st(float* p) const { *reinterpret_cast<float4*>(p) = q; }
    __device__ __forceinline__ void div(float d) { q.x = __fdiv_rn(q.x, d); q.y = __fdiv_rn(q.y, d); q.z = __fdiv_rn(q.z, d); q.w = __fdiv_rn(q.w, d); }
    __device__ __forceinline__ static Pix scaled(float w, const Pix& c) { return {make_float4(w * c.q.x, w * c.q.y, w * c.q.z, w * c.q.w)}; }
    __device__ __forceinline__ void tap(float w, const Pix& u, const Pix& v) {
        q.x = q.x + w * (u.q.x + v.q.x); q.y = q.y + w * (u.q.y + v.q.y); q.z = q.z + w * (u.q.z + v.q.z); q.w = q.w + w * (u.q.w + v.q.w);
    }
    __device__ __forceinline__ void step(float al, float b, const Pix& v) {
        q.x = al * q.x + b * v.q.x; q.y = al * q.y + b * v.q.y; q.z = al * q.z + b * v.q.z; q.w = al * q.w + b * v.q.w;
    }
};

// Output frames f0 .. f1 - 1 of one block, inside the frames lo_b .. hi_b that bound the reflections: the whole video (SHOTS false:
// 0 and F - 1, r <= F - 1, one bounce at most) or the run's shot (SHOTS true: any length, the walk bounces at either end as often
// as it must, and stands still in a shot of one frame).
template <bool MEAN, int V, bool SHOTS>
__device__ __forceinline__ void gauss_run(const VideoTemporalArgs& a, const int f0, const int f1, const int lo_b, const int hi_b) {
    using P = Pix<V>;
    extern __shared__ float4 ring_raw[];
    P* ring = reinterpret_cast<P*>(ring_raw);      // [2r + 1][GAUSS_TPB]
    constexpr int lanes = GAUSS_TPB;
    const int tid = threadIdx.x, r = a.r, R = 2 * r + 1;
    const long long p0 = (long long)blockIdx.x * lanes * V;
    const bool vec = V == 4 && (a.hw & 3) == 0 && aligned16(a.store, a.out);
    const long long mine = vec ? p0 + 4ll * tid : p0 + tid;      // V == 4, not vec: pixels mine + k * lanes
    if (mine >= a.hw) return;      // (no barrier below: a lane without pixels may leave)

    auto load = [&](int g) -> P {
        const float* src = a.store + (long long)g * a.hw;
        P v = P::zero();
        if constexpr (V == 4) {
            if (vec) v = P::ld(src + mine);
            else {
                v.q.x = src[mine];
                if (mine + lanes < a.hw) v.q.y = src[mine + lanes];
                if (mine + 2ll * lanes < a.hw) v.q.z = src[mine + 2ll * lanes];
                if (mine + 3ll * lanes < a.hw) v.q.w = src[mine + 3ll * lanes];
            }
        } else {
            v = P::ld(src + mine);
        }
        if (MEAN) {
            const int c = a.count[g];
            if (c != 1) v.div((float)c);
        }
        return v;
    };

    // the window of the run's first output: frames max(lo_b, f0 - r) .. min(hi_b, f0 + r); frame g lives in slot g mod R
    const int lo = max(lo_b, f0 - r), hi = min(hi_b, f0 + r);
    int slot = lo % R;
    for (int g = lo; g <= hi; g += GAUSS_PRELOAD) {
        P v[GAUSS_PRELOAD];
#pragma unroll
        for (int u = 0; u < GAUSS_PRELOAD; ++u)
            if (g + u <= hi) v[u] = load(g + u);
#pragma unroll
        for (int u = 0; u < GAUSS_PRELOAD; ++u)
            if (g + u <= hi) {
                ring[slot * lanes + tid] = v[u];
                if (++slot == R) slot = 0;
            }
    }
    int cs = f0 % R;      // the slot of frame f
    for (int f = f0; f < f1; ++f) {
        // frame f + r + 1 joins the window of output f + 1 and takes the slot of frame f - r, which output f still reads
        const int gn = f + r + 1;
        const bool more = f + 1 < f1 && gn <= hi_b;
        P nxt = P::zero();
        if (more) nxt = load(gn);
        P acc = P::scaled(a.w[0], ring[cs * lanes + tid]);
        int ja = f, jb = f, sa = cs, sb = cs, da = -1, db = 1;      // rho(f - d), rho(f + d) and their slots
        if (SHOTS && lo_b == hi_b) da = db = 0;
        for (int d = 1; d <= r; ++d) {
            if (SHOTS) {
                if (ja == lo_b && da < 0) da = 1; else if (ja == hi_b && da > 0) da = -1;
                if (jb == hi_b && db > 0) db = -1; else if (jb == lo_b && db < 0) db = 1;
            } else {
                if (ja == lo_b) da = 1;
                if (jb == hi_b) db = -1;
            }
            ja += da; sa += da;
            if (sa < 0) sa += R; else if (sa >= R) sa -= R;
            jb += db; sb += db;
            if (sb < 0) sb += R; else if (sb >= R) sb -= R;
            acc.tap(a.w[d], ring[sa * lanes + tid], ring[sb * lanes + tid]);
        }
        float* o = a.out + (long long)(f - a.first) * a.hw;
        if constexpr (V == 4) {
            if (vec) acc.st(o + mine);
            else {
                o[mine] = acc.q.x;
                if (mine + lanes < a.hw) o[mine + lanes] = acc.q.y;
                if (mine + 2ll * lanes < a.hw) o[mine + 2ll * lanes] = acc.q.z;
                if (mine + 3ll * lanes < a.hw) o[mine + 3ll * lanes] = acc.q.w;
            }
        } else {
            acc.st(o + mine);
        }
        if (more) {
            int ns = cs - r;
            if (ns < 0) ns += R;
            ring[ns * lanes + tid] = nxt;
        }
        if (++cs == R) cs = 0;
    }
}

template <bool MEAN, int V>
__global__ __launch_bounds__(GAUSS_TPB) void video_temporal_gauss_kernel(VideoTemporalArgs a, int fpb) {
    const int f0 = a.first + (int)blockIdx.y * fpb, f1 = min(f0 + fpb, a.first + a.n);
    gauss_run<MEAN, V, false>(a, f0, f1, 0, a.F - 1);
}

// Under a shot table: blockIdx.y is a run (f0, f1, lo, hi) of the table in scratch -- output frames f0 .. f1 - 1, all of them in the
// shot lo .. hi, so that no run straddles a cut and no frame of another shot is ever loaded.
template <bool MEAN, int V>
__global__ __launch_bounds__(GAUSS_TPB) void video_temporal_gauss_shots_kernel(VideoTemporalArgs a, const int* runs) {
    const int* run = runs + 4 * (size_t)blockIdx.y;
    gauss_run<MEAN, V, true>(a, run[0], run[1], run[2], run[3]);
}

template <bool MEAN, int V>
__global__ __launch_bounds__(EMA_TPB) void video_temporal_ema_kernel(VideoTemporalArgs a) {
    using E = Pix<V>;
    const long long i = ((long long)blockIdx.x * EMA_TPB + threadIdx.x) * V;
    if (i >= a.hw) return;
    const float al = a.alpha, b = 1.0f - al;
    const int end = a.first + a.n;      // frames 0 .. end - 1
    auto load = [&](int g) -> E {
        E v = E::ld(a.store + (long long)g * a.hw + i);
        if (MEAN) {
            const int c = a.count[g];
            if (c != 1) v.div((float)c);
        }
        return v;
    };
    auto store = [&](int f, const E& m) {
        if (f >= a.first) m.st(a.out + (long long)(f - a.first) * a.hw + i);
    };
    E m = load(0);
    store(0, m);
    int f = 1;
    for (; f + EMA_UNROLL <= end; f += EMA_UNROLL) {
        E v[EMA_UNROLL];
#pragma unroll
        for (int u = 0; u < EMA_UNROLL; ++u) v[u] = load(f + u);
#pragma unroll
        for (int u = 0; u < EMA_UNROLL; ++u) {
            m.step(al, b, v[u]);
            store(f + u, m);
        }
    }
    for (; f < end; ++f) {
        m.step(al, b, load(f));
        store(f, m);
    }
}

// Under a shot table: the runs are whole shots from their first frame (f0 == lo), the first of them the shot frame `first` lies
// in; the recurrence restarts with a copy of the bits at every run and nothing before `first` is stored.
template <bool MEAN, int V>
__global__ __launch_bounds__(EMA_TPB) void video_temporal_ema_shots_kernel(VideoTemporalArgs a, const int* runs, int n_runs) {
    using E = Pix<V>;
    const long long i = ((long long)blockIdx.x * EMA_TPB + threadIdx.x) * V;
    if (i >= a.hw) return;
    const float al = a.alpha, b = 1.0f - al;
    auto load = [&](int g) -> E {
        E v = E::ld(a.store + (long long)g * a.hw + i);
        if (MEAN) {
            const int c = a.count[g];
            if (c != 1) v.div((float)c);
        }
        return v;
    };
    auto store = [&](int f, const E& m) {
        if (f >= a.first) m.st(a.out + (long long)(f - a.first) * a.hw + i);
    };
    for (int k = 0; k < n_runs; ++k) {
        const int begin = runs[4 * k], end = runs[4 * k + 1];
        E m = load(begin);
        store(begin, m);
        int f = begin + 1;
        for (; f + EMA_UNROLL <= end; f += EMA_UNROLL) {
            E v[EMA_UNROLL];
#pragma unroll
            for (int u = 0; u < EMA_UNROLL; ++u) v[u] = load(f + u);
#pragma unroll
            for (int u = 0; u < EMA_UNROLL; ++u) {
                m.step(al, b, v[u]);
                store(f + u, m);
            }
        }
        for (; f < end; ++f) {
            m.step(al, b, load(f));
            store(f, m);
        }
    }
}

bool ema_vec(const VideoTemporalArgs& a) {
    return a.hw >= EMA_VEC_MIN_HW && (a.hw & 3) == 0 && ((((unsigned long long)a.store | (unsigned long long)a.out)) & 15ull) == 0;
}

bool temporal_ok(const VideoTemporalArgs& a, bool shots = false) {
    if (!a.store || !a.out || a.store == a.out) return false;
    if (a.F < 1 || a.hw < 1 || a.n < 1 || a.first < 0 || a.first > a.F - a.n) return false;
    if (a.kind == TEMPORAL_GAUSS) return a.r >= 1 && a.r <= TEMPORAL_MAX_RADIUS && (shots || a.r <= a.F - 1);      // the reflections stay inside the ring
    if (a.kind == TEMPORAL_EMA) return a.alpha >= 0.f && a.alpha < 1.f;
    return false;
}

}  // namespace

VideoTemporalPlan p3d_video_temporal_plan(int kind, int r, long long hw, int n) {
    VideoTemporalPlan p;
    if (kind == TEMPORAL_EMA) {
        p.threads = EMA_TPB;
        p.pixels_per_block = EMA_TPB * ((hw >= EMA_VEC_MIN_HW && (hw & 3) == 0) ? 4 : 1);
        p.frames_per_block = n;
        p.lds_bytes = 0;
        return p;
    }
    // GAUSS: four pixels a lane while the ring of 2r + 1 inputs fits 64 KB, else one.  A run long enough that about
    // GAUSS_TARGET_BLOCKS blocks share the read, and not shorter than r (or GAUSS_MIN_RUN), so that a run's halo at most
    // triples its loads
    const int R = 2 * r + 1;
    const int V = R * GAUSS_TPB * 16 <= GAUSS_LDS_MAX ? 4 : 1;
    p.threads = GAUSS_TPB;
    p.pixels_per_block = GAUSS_TPB * V;
    p.lds_bytes = R * GAUSS_TPB * 4 * V;
    const long long strips = (hw + p.pixels_per_block - 1) / p.pixels_per_block;
    const long long runs = std::max<long long>(1, GAUSS_TARGET_BLOCKS / strips);
    long long fpb = std::max<long long>((n + runs - 1) / runs, std::min<long long>(n, std::max(r, GAUSS_MIN_RUN)));
    fpb = std::max<long long>(fpb, ((long long)n + 65534) / 65535);      // gridDim.y
    p.frames_per_block = (int)std::max<long long>(1, std::min<long long>(fpb, n));
    return p;
}

LaunchDesc p3d_video_temporal_desc(const VideoTemporalArgs& a) {
    const bool mean = a.count != nullptr;
    if (a.kind == TEMPORAL_EMA) {
        const double in = (double)a.first + a.n;
        return {mean ? "video_temporal_ema_kernel<1>" : "video_temporal_ema_kernel<0>", 3.0 * (in - 1.0) * (double)a.hw,
                (in + (double)a.n) * (double)a.hw * 4.0};
    }
    // every run loads its own frames and the r either side that exist
    const int fpb = p3d_video_temporal_plan(a.kind, a.r, a.hw, a.n).frames_per_block;
    double in = 0.0;
    for (int f0 = a.first; f0 < a.first + a.n; f0 += fpb) {
        const int f1 = std::min(f0 + fpb, a.first + a.n);
        in += std::min(a.F - 1, f1 - 1 + a.r) - std::max(0, f0 - a.r) + 1;
    }
    return {mean ? "video_temporal_gauss_kernel<1>" : "video_temporal_gauss_kernel<0>", (1.0 + 3.0 * a.r) * (double)a.n * (double)a.hw,
            (in + (double)a.n) * (double)a.hw * 4.0};
}

hipError_t p3d_video_temporal_launch(const VideoTemporalArgs& a, hipStream_t s) {
    if (!temporal_ok(a)) return hipErrorInvalidValue;
    const bool mean = a.count != nullptr;
    const VideoTemporalPlan p = p3d_video_temporal_plan(a.kind, a.r, a.hw, a.n);
    if (a.kind == TEMPORAL_EMA) {
        const bool v4 = ema_vec(a);
        const long long lanes = v4 ? a.hw / 4 : a.hw, blocks = (lanes + EMA_TPB - 1) / EMA_TPB;
        if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
        const dim3 grid((unsigned)blocks);
        if (mean && v4) hipLaunchKernelGGL((video_temporal_ema_kernel<true, 4>), grid, dim3(EMA_TPB), 0, s, a);
        else if (mean) hipLaunchKernelGGL((video_temporal_ema_kernel<true, 1>), grid, dim3(EMA_TPB), 0, s, a);
        else if (v4) hipLaunchKernelGGL((video_temporal_ema_kernel<false, 4>), grid, dim3(EMA_TPB), 0, s, a);
        else hipLaunchKernelGGL((video_temporal_ema_kernel<false, 1>), grid, dim3(EMA_TPB), 0, s, a);
        return hipGetLastError();
    }
    const long long strips = (a.hw + p.pixels_per_block - 1) / p.pixels_per_block;
    const int runs = (a.n + p.frames_per_block - 1) / p.frames_per_block;
    if (strips > 0x7fffffffll || runs > 65535 || p.lds_bytes > GAUSS_LDS_MAX) return hipErrorInvalidValue;
    const dim3 grid((unsigned)strips, (unsigned)runs);
    const bool v4 = p.pixels_per_block == 4 * GAUSS_TPB;
    if (mean && v4) hipLaunchKernelGGL((video_temporal_gauss_kernel<true, 4>), grid, dim3(GAUSS_TPB), p.lds_bytes, s, a, p.frames_per_block);
    else if (mean) hipLaunchKernelGGL((video_temporal_gauss_kernel<true, 1>), grid, dim3(GAUSS_TPB), p.lds_bytes, s, a, p.frames_per_block);
    else if (v4) hipLaunchKernelGGL((video_temporal_gauss_kernel<false, 4>), grid, dim3(GAUSS_TPB), p.lds_bytes, s, a, p.frames_per_block);
    else hipLaunchKernelGGL((video_temporal_gauss_kernel<false, 1>), grid, dim3(GAUSS_TPB), p.lds_bytes, s, a, p.frames_per_block);
    return hipGetLastError();
}

std::vector<int> p3d_video_temporal_runs(int kind, int r, long long hw, int F, int first, int n, const int32_t* starts, int n_shots) {
    std::vector<int> runs;
    const int last = first + n - 1;
    const int fpb = kind == TEMPORAL_GAUSS ? p3d_video_temporal_plan(kind, r, hw, n).frames_per_block : 0;
    for (int k = 0; k < n_shots; ++k) {
        const int lo = starts[k], hi = (k + 1 < n_shots ? starts[k + 1] : F) - 1;
        if (hi < first || lo > last) continue;
        if (kind == TEMPORAL_EMA) {
            runs.insert(runs.end(), {lo, std::min(hi, last) + 1, lo, hi});
            continue;
        }
        for (int f0 = std::max(first, lo); f0 <= std::min(last, hi); f0 += fpb) runs.insert(runs.end(), {f0, std::min(f0 + fpb, std::min(last, hi) + 1), lo, hi});
    }
    return runs;
}

hipError_t p3d_video_temporal_shots_launch(const VideoTemporalArgs& a, const int* runs, int n_runs, hipStream_t s) {
    if (!temporal_ok(a, true) || !runs || n_runs < 1) return hipErrorInvalidValue;
    const bool mean = a.count != nullptr;
    const VideoTemporalPlan p = p3d_video_temporal_plan(a.kind, a.r, a.hw, a.n);
    if (a.kind == TEMPORAL_EMA) {
        const bool v4 = ema_vec(a);
        const long long lanes = v4 ? a.hw / 4 : a.hw, blocks = (lanes + EMA_TPB - 1) / EMA_TPB;
        if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
        const dim3 grid((unsigned)blocks);
        if (mean && v4) hipLaunchKernelGGL((video_temporal_ema_shots_kernel<true, 4>), grid, dim3(EMA_TPB), 0, s, a, runs, n_runs);
        else if (mean) hipLaunchKernelGGL((video_temporal_ema_shots_kernel<true, 1>), grid, dim3(EMA_TPB), 0, s, a, runs, n_runs);
        else if (v4) hipLaunchKernelGGL((video_temporal_ema_shots_kernel<false, 4>), grid, dim3(EMA_TPB), 0, s, a, runs, n_runs);
        else hipLaunchKernelGGL((video_temporal_ema_shots_kernel<false, 1>), grid, dim3(EMA_TPB), 0, s, a, runs, n_runs);
        return hipGetLastError();
    }
    const long long strips = (a.hw + p.pixels_per_block - 1) / p.pixels_per_block;
    if (strips > 0x7fffffffll || p.lds_bytes > GAUSS_LDS_MAX) return hipErrorInvalidValue;
    const bool v4 = p.pixels_per_block == 4 * GAUSS_TPB;
    for (int k0 = 0; k0 < n_runs; k0 += 65535) {            // gridDim.y
        const dim3 grid((unsigned)strips, (unsigned)std::min(65535, n_runs - k0));
        const int* at = runs + 4 * (size_t)k0;
        if (mean && v4) hipLaunchKernelGGL((video_temporal_gauss_shots_kernel<true, 4>), grid, dim3(GAUSS_TPB), p.lds_bytes, s, a, at);
        else if (mean) hipLaunchKernelGGL((video_temporal_gauss_shots_kernel<true, 1>), grid, dim3(GAUSS_TPB), p.lds_bytes, s, a, at);
        else if (v4) hipLaunchKernelGGL((video_temporal_gauss_shots_kernel<false, 4>), grid, dim3(GAUSS_TPB), p.lds_bytes, s, a, at);
        else hipLaunchKernelGGL((video_temporal_gauss_shots_kernel<false, 1>), grid, dim3(GAUSS_TPB), p.lds_bytes, s, a, at);
    }
    return hipGetLastError();
}
