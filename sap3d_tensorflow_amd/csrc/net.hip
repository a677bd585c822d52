// Host runtime of libp3dhip: builds the P3D graph once (static shapes, everything resident in
// HBM), then runs forward / backward / Adam as a fixed list of kernel launches on one HIP stream,
// with RCCL gradient all-reduce on a side stream.  Graph structure follows the reference's
// graph-building functions (p3d.py:10-221) but nothing else of TF's runtime is mirrored: there is
// no session, no tracing, no host-resident variables.
//
// Parameters live in ONE flat fp32 buffer in creation (= forward) order with matching flat
// gradient / Adam-moment buffers, so the optimiser is one kernel and gradient buckets for the
// all-reduce are contiguous ranges that complete back-to-front during backward.
#include "../../include/p3d_hip.h"
#include "p3d_kernels.h"

#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

namespace {

thread_local std::string g_err;

// The product's own runtime switches (everything else is a -DP3D_TUNING switch, p3d_tune_env): read once.
struct RuntimeEnv { bool debug_sync = false, graph = false, no_side_stream = false; };
const RuntimeEnv& runtime_env() {
    static const RuntimeEnv env = [] {
        RuntimeEnv e;
        e.debug_sync = getenv("P3D_DEBUG_SYNC") != nullptr;                                   // synchronise and log after every op
        if (const char* v = getenv("P3D_GRAPH")) e.graph = atoi(v) != 0 && !e.debug_sync;      // captured step graph (slower on ROCm 7.2)
        e.no_side_stream = getenv("P3D_NO_SIDE_STREAM") != nullptr;                            // everything on one stream
        return e;
    }();
    return env;
}
// all-reduce bucket size in MB (also fixes where queued filter gradients are flushed); read whenever a handle or a communicator
// is created, so that one process can build handles with different bucket sizes (tests/test_gpu_dp.py); 0: the default
long bucket_mb_env() { const char* e = getenv("P3D_BUCKET_MB"); return e ? atol(e) : 0; }

struct P3dError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

#define HIPCHECK(expr)                                                                               \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess)                                                                        \
            throw P3dError(std::string(#expr) + " failed: " + hipGetErrorString(e_) + " (" __FILE__ ":" + \
                           std::to_string(__LINE__) + ")");                                          \
    } while (0)
#define NCCLCHECK(expr)                                                                              \
    do {                                                                                             \
        ncclResult_t r_ = (expr);                                                                    \
        if (r_ != ncclSuccess) throw P3dError(std::string(#expr) + " failed: " + ncclGetErrorString(r_)); \
    } while (0)

#include "dev_mem.inc"

enum InitKind { INIT_XAVIER = 0, INIT_ZEROS = 1, INIT_ONES = 2, INIT_VS = 3 };

struct Param {
    std::string name;
    std::vector<int64_t> shape;
    int64_t count = 0, off = 0;
    bool trainable = true;
    int init = INIT_XAVIER;
    float* p = nullptr;     // device
    float* g = nullptr;     // device gradient (trainables)
    int reg = 0;            // regularisation class, P3D_REG_*: what the reference's graph build adds to its collections
};

// The stem: conv -> BatchNorm -> ReLU, and the conv has no input gradient.  The normalisation's backward then ends after its
// reduce / finalize launches and hands its arguments to the conv's filter gradient, which applies it on its operand path.
struct StemBnLink {
    bool enabled = false, pending = false; BnBwdArgs args;
    std::vector<const Param*> reads;      // variables the filter gradient reads when it takes the apply pass (the BatchNorm's gamma)
};

struct Act {
    std::string name;
    int N = 0, D = 0, H = 0, W = 0, C = 0, ld = 0;
    float* p = nullptr;
    float* g = nullptr;
    Act* parent = nullptr;          // channel-slice view of parent's storage
    std::vector<Act*> views;
    char* last_flag = nullptr;      // accumulate-flag of the most recently registered consumer
    bool whole_consumed = false;    // a consumer of the whole buffer (all views) is registered
    // BatchNorm fusion: a normalised tensor that the fused forward never stores; reading it (p3d_get_activation) runs this
    std::function<void(hipStream_t)> materialize;
    // the stem conv's output: its BatchNorm's backward may leave the apply pass to the conv's filter gradient (stem_wgrad.hip)
    std::shared_ptr<struct StemBnLink> stem_link;
    int64_t rows() const { return (int64_t)N * D * H * W; }
};

struct BN {
    std::string name;
    int C = 0;
    Param *gamma = nullptr, *beta = nullptr, *mm = nullptr, *mv = nullptr;
    int64_t part_off = -1;          // statistics partials [part_cap][C][2] floats in statpart_arena (-1: producer has no epilogue)
    int part_cap = 0;
    int nparts = 0;                 // partials the last forward's producer wrote (host-side, set at enqueue)
    float *scale = nullptr, *shift = nullptr, *mean = nullptr, *invstd = nullptr;
    bool follows_flag = false;      // obeys the `training` placeholder (stem / decoder); else always batch stats
    bool used_batch = true;         // what the last forward used
    // BatchNorm fusion (p3d_kernels.h): backward partials (sum g, sum g*xhat) per output tile of the gating launch, and the
    // published k1 / k2 / k3 of dy = k1*g + k2*y + k3
    bool fusable = false;
    int64_t gpart_off = -1; int gpart_cap = 0; int gnparts = 0;
    float* coef = nullptr;
};

// Per-launch HIP-event timing (p3d_profile_step): one record per kernel launch, on the launch stream.
struct ProfRec {
    std::string kernel, op;
    double flops = 0, bytes = 0;
    int phase = 0;                 // 0 forward, 1 backward, 2 optimiser
    hipEvent_t e0 = nullptr, e1 = nullptr;
};
struct Prof {
    std::vector<ProfRec> recs;
    int phase = 0;
    std::string cur_op;
};

struct GN {                            // one GroupNorm layer (gn/p3d_gn.py:24-46)
    std::string name;
    int C = 0, G = 0, N = 0;
    Param *gamma = nullptr, *beta = nullptr;
    int64_t sums_off = 0;              // forward (sum, sumsq) in the stats arena   [N][C][2] doubles
    int64_t bsums_off = 0;             // backward sums in the reduction arena       [N][C][2] doubles
    int64_t tab_off = 0;               // scale, shift, mean, invstd [N][C] each + coef [N][C][3], in bnbuf
};

struct CbamSite {                      // one cbam_block on a bottleneck residual (utils/network.py:198-274)
    Param *k0 = nullptr, *b0 = nullptr, *k1 = nullptr, *b1 = nullptr, *k7 = nullptr;
    Act* x = nullptr;
    float* dout = nullptr;             // gradient of the CBAM output, written by the block-end pass
    int chunks = 1;
    int64_t buf_off = 0;               // float scratch in bnbuf
    char* xflag = nullptr;
};

struct Ctx {
    bool training = false;
    float drop = 0.f;
    uint64_t seed = 0;
    const unsigned long long* seed_dev = nullptr;   // captured step graphs: dropout seed and Adam step size live in device memory
    const float* lr_dev = nullptr;
    const float* om_dev = nullptr;    // ... and the moving average's om under warm-up (p3d_set_ema)
    bool acc_finish = false;          // the applying micro-step of p3d_set_grad_accum: the backward finishes flat_g = acc + g
    bool update_moving = false;
    bool per_sample = false;          // batch-statistics BNs normalise every clip by its own statistics (p3d_predict_windows)
    bool fuse = false;                // BatchNorm fused into the neighbouring convs' operand paths (set by run_forward / run_backward)
    bool fuse_bwd = false;            // ... in the backward pass as well (else: BatchNorm's backward keeps its own launches)
    hipStream_t s = nullptr;
    Prof* prof = nullptr;
    hipStream_t side = nullptr;       // weight gradients run here, off the backward critical path
    // planning pass (finalize_build): nothing is launched, zero-fill requests are recorded instead
    std::vector<std::pair<float*, size_t>>* dry = nullptr;
    // buffers inside [z0, z1) are zeroed wholesale at the start of the phase: no per-op memset
    const char* z0 = nullptr; const char* z1 = nullptr;
    // backward of the decoder: side-stream jobs are parked here and released when the walk reaches the encoder (run_backward)
    std::vector<std::pair<hipEvent_t, std::function<void(const Ctx&)>>>* defer = nullptr;
    const char* bwd_op = nullptr;     // name of the op whose backward is running (diagnostics)
};

// ---- schedule trace (test hook p3d_debug_schedule): every stream operation of a pass -- kernel launches, async fills, event
//      records and waits, all-reduce launches -- in host issue order, with streams and events named by small ids.  The ordering
//      bugs this file can have (a fill that is not ordered against the launch behind it, a hand-over before its producer) do
//      not show as numbers until another session reuses the state; they do show in who waits for whom.
struct SchedTrace {
    std::vector<std::string> lines;
    std::map<hipStream_t, std::string> streams;
    std::map<hipEvent_t, int> events;
    std::string sname(hipStream_t s) {
        auto it = streams.find(s);
        if (it != streams.end()) return it->second;
        const std::string n = "s" + std::to_string(streams.size());
        streams[s] = n;
        return n;
    }
    int eid(hipEvent_t e) {
        auto it = events.find(e);
        if (it != events.end()) return it->second;
        const int n = (int)events.size();
        events[e] = n;
        return n;
    }
};
thread_local SchedTrace* g_trace = nullptr;
// ---- schedule perturbation (test hook p3d_debug_perturb, tests/test_gpu_stream_hazards.py): the step is bit-reproducible by design,
//      so a correct schedule gives the same bits however its streams drift against each other.  serial: the issuing stream is
//      synchronised after every launch, fill and all-reduce -- the host's issue order, one legal order.  slow: a bounded delay
//      kernel (elementwise.hip, p3d_delay) goes onto ONE stream ahead of everything issued there, so the others run ahead as far
//      as the events allow: a slow producer shows a consumer that lacks its wait, a slow consumer a buffer that is reused under
//      it.  Only the three streams of the handle the hook was set on are touched; the delay kernels are not traced.  Set per
//      calling thread, like g_trace; off (the default), launch() pays one thread-local null check.
struct Perturb {
    int mode = 0;                              // 0 off, 1 serial, 2 slow
    hipStream_t streams[3] = {nullptr, nullptr, nullptr};      // main, side, comm
    hipStream_t target = nullptr;              // slow: the stream that is held back
    int delay_us = 0;
    int64_t delays = 0, syncs = 0;             // inserted since the hook was last set
    hipError_t before(hipStream_t s) {
        if (mode != 2 || s != target) return hipSuccess;
        ++delays;
        return p3d_delay(delay_us, s);
    }
    hipError_t after(hipStream_t s) {
        if (mode != 1 || (s != streams[0] && s != streams[1] && s != streams[2])) return hipSuccess;
        ++syncs;
        return hipStreamSynchronize(s);
    }
};
thread_local Perturb* g_perturb = nullptr;
struct PerturbPause {                          // profiling passes time single launches: the hook stays out of them
    Perturb* const saved = g_perturb;
    PerturbPause() { g_perturb = nullptr; }
    ~PerturbPause() { g_perturb = saved; }
};
inline hipError_t ev_record(hipEvent_t e, hipStream_t s) {
    if (g_trace) g_trace->lines.push_back("R " + g_trace->sname(s) + " e" + std::to_string(g_trace->eid(e)));
    return hipEventRecord(e, s);
}
inline hipError_t ev_wait(hipStream_t s, hipEvent_t e) {
    if (g_trace) g_trace->lines.push_back("W " + g_trace->sname(s) + " e" + std::to_string(g_trace->eid(e)));
    return hipStreamWaitEvent(s, e, 0);
}
// Every fill and copy of this library NAMES ITS STREAM (round 5).  A bare hipMemset / hipMemcpy runs on the null stream, which
// is not ordered against the handle's non-blocking streams: twice in two rounds such a call raced a launch (arrival counters
// zeroed under a running kernel; decision-hook scratch zeroed while its gate kernels ran).  fill_now / copy_now enqueue on the
// given stream and wait for it, so they are ordered after everything queued there and complete on return;
// tests/test_abi_cpu.py fails on any other spelling in csrc/.
inline hipError_t fill_now(void* p, int v, size_t bytes, hipStream_t s) {
    const hipError_t e = hipMemsetAsync(p, v, bytes, s);
    return e != hipSuccess ? e : hipStreamSynchronize(s);
}
inline hipError_t copy_now(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
    const hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, s);
    return e != hipSuccess ? e : hipStreamSynchronize(s);
}
inline hipError_t fill_async(void* p, int v, size_t bytes, hipStream_t s, const char* what) {
    if (g_trace) g_trace->lines.push_back("M " + g_trace->sname(s) + " " + what);
    Perturb* const pt = g_perturb;
    if (!pt) return hipMemsetAsync(p, v, bytes, s);
    hipError_t e = pt->before(s);
    if (e == hipSuccess) e = hipMemsetAsync(p, v, bytes, s);
    return e != hipSuccess ? e : pt->after(s);
}

template <typename F>
void launch(const Ctx& c, const char* kernel, double flops, double bytes, F&& f) {
    if (c.dry) return;
    if (g_trace) g_trace->lines.push_back("L " + g_trace->sname(c.s) + " " + kernel + (c.bwd_op ? std::string(" @") + c.bwd_op : std::string()));
    if (!c.prof) {
        Perturb* const pt = g_perturb;
        if (pt) HIPCHECK(pt->before(c.s));
        HIPCHECK(f());
        if (pt) HIPCHECK(pt->after(c.s));
        return;
    }
    ProfRec r;
    r.kernel = kernel; r.op = c.prof->cur_op; r.flops = flops; r.bytes = bytes; r.phase = c.prof->phase;
    HIPCHECK(hipEventCreate(&r.e0));
    HIPCHECK(hipEventCreate(&r.e1));
    HIPCHECK(hipEventRecord(r.e0, c.s));
    HIPCHECK(f());
    HIPCHECK(hipEventRecord(r.e1, c.s));
    c.prof->recs.push_back(r);
}

std::atomic<int> g_live_handles{0};      // p3d_create .. p3d_destroy; p3d_shutdown refuses while any is alive

// ---- stream pool (round 5) ------------------------------------------------------------------------------------------------------
// A handle needs three streams (main and comm at the highest priority, side at the lowest).  A process that opens and closes many
// handles -- the test suite: ~250 sessions -- used to create and destroy three hardware queues per handle; the runtime releases
// them lazily, and one full-suite run of round 5 died with a bare abort() inside p3d_create after 235 tests (no message, not
// reproduced in two further runs).  Streams are now returned to a per-device, per-priority pool by p3d_destroy and taken from it
// by p3d_create: a long-lived process keeps three queues per device however many handles it has seen, and the K-slice scratch,
// which is keyed by stream, is reused with them instead of accumulating per session.  p3d_shutdown destroys the pooled streams.
struct StreamPool {
    std::mutex m;
    std::map<std::pair<int, int>, std::vector<hipStream_t>> idle;      // (device, priority class: 0 highest, 1 lowest)
};
StreamPool& stream_pool() { static StreamPool p; return p; }
hipStream_t take_stream(int device, int prio_class) {
    {
        std::lock_guard<std::mutex> g(stream_pool().m);
        auto& v = stream_pool().idle[{device, prio_class}];
        if (!v.empty()) { hipStream_t s = v.back(); v.pop_back(); return s; }
    }
    int least = 0, greatest = 0;
    HIPCHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    hipStream_t s = nullptr;
    HIPCHECK(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, prio_class == 0 ? greatest : least));
    return s;
}
void give_stream(int device, int prio_class, hipStream_t s) {      // the stream must be idle (p3d_destroy synchronises the device first)
    if (!s) return;
    std::lock_guard<std::mutex> g(stream_pool().m);
    stream_pool().idle[{device, prio_class}].push_back(s);
}
void destroy_pooled_streams() {
    std::lock_guard<std::mutex> g(stream_pool().m);
    for (auto& kv : stream_pool().idle)
        for (hipStream_t s : kv.second) hipStreamDestroy(s);
    stream_pool().idle.clear();
}
const float* g_zero_page = nullptr;      // 1 KiB of zeros (device), set by p3d_create / op entry points

void igemm_work(const IgemmArgs& a, double& flops, double& bytes) {
    const double M = (double)a.N * a.Gd * a.Gh * a.Gw;
    const double side = (double)a.N * a.Di * a.Hi * a.Wi;
    const double gathered = std::min(M * std::max(a.ntaps, 1), side);
    flops = 2.0 * M * a.ntaps * (double)a.K * a.Nc;
    bytes = 4.0 * (gathered * a.K + M * a.Nc * (1 + a.accum) + (double)a.ntaps * a.K * a.Nc);
}

void launch_igemm(const Ctx& c, const IgemmArgs& a0, int allow_split = 0) {
    IgemmArgs a = a0;
    double fl, by;
    igemm_work(a, fl, by);
    a.zeros = g_zero_page;
    const P3dIgemmPlan pl = p3d_igemm2_plan(a, allow_split);
    const char* name = pl.name;
    if (a.f16) name = pl.bm == 128 ? (pl.bn == 128 ? "igemm2_kernel<128,128,f16>" : "igemm2_kernel<128,64,f16>") : "igemm2_kernel<64,64,f16>";
    else if (a.at_mode || a.ngate) {      // fused-BatchNorm variants get their own rows in the per-kernel tables
        static const char* const tiles[3] = {"64,64", "128,64", "128,128"};
        static const char* const ats[4] = {"", ",relu1", ",relu2", ",bngrad"};
        static std::map<int, std::string> names;
        const int key = (pl.bm == 128 ? (pl.bn == 128 ? 2 : 1) : 0) * 8 + a.at_mode * 2 + (a.ngate ? 1 : 0);
        std::string& nm = names[key];
        if (nm.empty()) nm = std::string("igemm2_kernel<") + tiles[key / 8] + ats[a.at_mode] + (a.ngate ? ",gate" : "") + ">";
        name = nm.c_str();
    }
    launch(c, name, fl, by, [&]() { return p3d_launch_igemm2(a, pl, c.s); });
}

void zero_strided(const Ctx& c, float* p, int ld, int64_t rows, int C);

// Where a producer's BatchNorm-statistics epilogue puts its per-tile partial sums, and how many it wrote
// (read by p3d_bn_finalize right after, on the same stream).
struct StatSink { float* part = nullptr; int cap = 0; int* nparts = nullptr; };

// Room for the statistics partials of a `rows` x C output, whichever producer writes them: one per 64-row tile of every
// launch of the group (residue classes of a transposed conv: up to 64), one per block of p3d_bn_stats, or one per block
// of the streaming 1x1x1 kernel (conv_pointwise.hip: up to 512 from 16 384 rows on, 32-row slabs at 128 channels).
int bn_part_cap(int64_t rows, int C) {
    return (int)std::max<int64_t>({rows / 64 + 80, (int64_t)p3d_bn_stats_parts((long)rows, C), (int64_t)p3d_pw_stream_max_blocks(rows, C)});
}

// One grouped launch of `v` (conv_igemm2.hip, igemm2_group_kernel) with the summed work of its members.
void launch_igemm_group(const Ctx& c, std::vector<IgemmArgs>& v, const P3dIgemmPlan& pl, const char* suffix) {
    double fl = 0, by = 0;
    for (auto& a : v) { double f1, b1; igemm_work(a, f1, b1); fl += f1; by += b1; }
    const std::string kn = "igemm2_group_kernel<" + std::to_string(pl.bm) + "," + std::to_string(pl.bn) + ">" + suffix;
    launch(c, kn.c_str(), fl, by, [&]() { return p3d_launch_igemm2_group(v.data(), (int)v.size(), pl, c.s); });
}

// A group of implicit-GEMM launches that together produce one output tensor (one conv forward,
// or the residue classes of an input gradient / transposed conv).  Small problems slice K across blocks;
// the slices are folded in a fixed order by the last arriving block (conv_igemm2.hip), so the output needs no
// zero fill and the statistics epilogue and accumulate mode work either way.
// fork / join non-null: the launches are independent (residue classes of a transposed conv write disjoint output
// positions) and each of them leaves CUs idle (196 blocks of 128x128 on 256 CUs): odd ones go to the side stream so that
// two classes run at a time.
void run_igemm_group(const Ctx& c, std::vector<IgemmArgs>& v, bool accumulate, const StatSink* stats, hipEvent_t fork = nullptr,
                     hipEvent_t join = nullptr) {
    int base = 0;
    for (auto& a : v) {
        a.accum = accumulate ? 1 : 0;
        a.statpart = nullptr; a.stat_base = 0;
        a.zeros = g_zero_page;
        if (stats && stats->part) {
            const P3dIgemmPlan pl = p3d_igemm2_plan(a, 1);
            const int mt = p3d_igemm2_mtiles(a, pl);
            if (base + mt > stats->cap) throw P3dError("statistics partials overflow their arena slot");
            a.statpart = stats->part; a.stat_base = base;
            base += mt;
        }
    }
    // residue classes that share a plan go out as ONE launch (conv_igemm2.hip, igemm2_group_kernel): a class alone leaves
    // CUs idle (deconv3 at 8 clips: 196 tiles of 128x128 per class), all of them together fill the chip in a few waves
    if (v.size() >= 2 && !c.dry) {
        const P3dIgemmPlan pl = p3d_igemm2_plan(v[0], 1);
        if (p3d_igemm2_groupable(v.data(), (int)v.size(), pl)) {
            launch_igemm_group(c, v, pl, "");
            if (stats && stats->nparts) *stats->nparts = base;
            return;
        }
    }
    const bool spread = fork && join && c.side && !c.dry && !c.prof && v.size() >= 4;
    Ctx sc = c;
    if (spread) {
        sc.s = c.side;
        HIPCHECK(ev_record(fork, c.s));
        HIPCHECK(ev_wait(c.side, fork));
    }
    int index = 0;
    for (auto& a : v) {
        launch_igemm((spread && (index & 1)) ? sc : c, a, 1);
        ++index;
    }
    if (spread) {
        HIPCHECK(ev_record(join, c.side));
        HIPCHECK(ev_wait(c.s, join));
    }
    if (stats && stats->nparts) *stats->nparts = base;
}

// Sibling convs on one input (ST_B, net_ops.inc conv()): each is a fresh launch that writes its statistics partials into its
// own BatchNorm's slot from partial 0 (unlike a residue-class group, which stacks its bases) ...
void sibling_prepare(IgemmArgs& a, const StatSink* sink) {
    a.zeros = g_zero_page; a.accum = 0; a.statpart = nullptr; a.stat_base = 0;
    if (!sink) return;
    const int mt = p3d_igemm2_mtiles(a, p3d_igemm2_plan(a, 1));
    if (mt > sink->cap) throw P3dError("statistics partials overflow their arena slot");
    a.statpart = sink->part; *sink->nparts = mt;
}
// ... and the pair goes out as ONE grouped launch when the plan allows it (either alone leaves most CUs idle), else as one
// launch each.  Returns whether it was grouped.
bool launch_siblings(const Ctx& c, std::vector<IgemmArgs>& v) {
    const P3dIgemmPlan pl = p3d_igemm2_plan(v[0], 1);
    if (p3d_igemm2_groupable(v.data(), (int)v.size(), pl)) {
        launch_igemm_group(c, v, pl, "(siblings)");
        return true;
    }
    for (auto& q : v) launch_igemm(c, q, 1);
    return false;
}

// tf.train.AdamOptimizer's bias-corrected step size lr * sqrt(1 - b2^t) / (1 - b1^t) for step t (train.py:168), in double from
// the float hyper-parameters; the network's optimiser step and the test hook p3d_debug_adam both take it from here.
float adam_step_size(float lr, float b1, float b2, int64_t t_step) {
    const double t = (double)t_step;
    return (float)(lr * std::sqrt(1.0 - std::pow((double)b2, t)) / (1.0 - std::pow((double)b1, t)));
}

// The dropout fields of a launch's arguments (every struct names them alike): left zero unless the site drops out and the pass trains.
template <typename Args>
void set_dropout(Args& a, const Ctx& c, bool dropout) {
    if (dropout && c.training && c.drop > 0.f) { a.drop_rate = c.drop; a.drop_scale = 1.f / (1.f - c.drop); a.seed = c.seed; a.seed_dev = c.seed_dev; }
}

// A GroupNorm's parameters, sums [N][C][2] and table: scale, shift, mean, invstd [N][C] each, then coef [N][C][3] (only here).
GnParams gn_layout(const float* gamma, const float* beta, double* sums, float* tab, int N, int C, int G) {
    GnParams p;
    const int64_t nc = (int64_t)N * C;
    p.gamma = gamma; p.beta = beta; p.sums = sums; p.C = C; p.G = G;
    p.scale = tab; p.shift = tab + nc; p.mean = tab + 2 * nc; p.invstd = tab + 3 * nc; p.coef = tab + 4 * nc;
    return p;
}
// One operand of a GroupNorm pass: values, where their gradient goes and, if it is normalised, its GroupNorm's layout (forward or
// backward sums) and parameter gradients.  With them, the kernels' arguments (gn_apply in net_gn.inc, the hook p3d_debug_gn_pass).
struct GnOperand {
    const float* y = nullptr; int ld = 0; float* dy = nullptr; int lddy = 0;
    GnParams g = {}; float* dgamma = nullptr; float* dbeta = nullptr;
};
GnApplyArgs gn_apply_args(int mode, int64_t M, int R, int C, float eps, const GnOperand& o1, const GnOperand& o2, int acc2,
                          const float* cs, const float* ss, float* z, int ldz, const float* dz, const Ctx& c, bool dropout) {
    GnApplyArgs a;
    memset(&a, 0, sizeof(a));
    a.mode = mode; a.M = M; a.R = R; a.C = C;
    a.y1 = o1.y; a.ld1 = o1.ld; a.g1 = o1.g; a.dy1 = o1.dy; a.lddy1 = o1.lddy; a.dgamma1 = o1.dgamma; a.dbeta1 = o1.dbeta;
    a.y2 = o2.y; a.ld2 = o2.ld; a.g2 = o2.g; a.dy2 = o2.dy; a.lddy2 = o2.lddy; a.dgamma2 = o2.dgamma; a.dbeta2 = o2.dbeta; a.acc2 = acc2;
    a.cs = cs; a.ss = ss; a.z = z; a.ldz = ldz; a.dz = dz; a.eps = eps;
    set_dropout(a, c, dropout);
    return a;
}

// One GroupNorm pass: which kernels take it, and their launches.  A (sample, group) slab that fits one block goes to the one-launch
// small-tensor kernels unless the pass drops out, its two GroupNorms (G2 != 0) group differently or it is mode 2 (per-sample
// BatchNorm); everything else runs statistics -> finalize -> apply forward and reduce -> finalize (+ parameter gradients) -> apply backward.
bool gn_small_rule(int mode, int R, int C, int G1, int G2, bool dropout) {
    static const bool no_small = p3d_tune_env("P3D_NO_GN_SMALL") != nullptr;
    return !no_small && mode != 2 && !dropout && p3d_gn_small_ok(R, C, G1) && (!G2 || G2 == G1);
}
void gn_pass_forward(const Ctx& c, const GnApplyArgs& a, bool small) {
    const double tens = (double)a.M * a.C * 4.0;
    const int R = a.R, C = a.C, N = (int)(a.M / a.R), io = a.y2 ? 3 : 2;
    if (small) {
        const std::string ksf = "gn_small_fwd_kernel<" + std::to_string(a.mode) + ">";
        launch(c, ksf.c_str(), 0, tens * io, [&]() { return p3d_gn_small_fwd(a, c.s); });
        return;
    }
    const std::string ka = "gn_apply_kernel<" + std::to_string(a.mode) + ">";
    launch(c, "gn_stats_kernel", 0, tens, [&]() { return p3d_gn_stats(a.y1, a.ld1, N, R, C, a.g1.sums, c.s); });
    launch(c, "gn_finalize_kernel", 0, 32.0 * N * C, [&]() { return p3d_gn_finalize(a.g1, N, R, a.eps, c.s); });
    if (a.mode == 2 || a.mode == 3) {
        launch(c, "gn_stats_kernel", 0, tens, [&]() { return p3d_gn_stats(a.y2, a.ld2, N, R, C, a.g2.sums, c.s); });
        launch(c, "gn_finalize_kernel", 0, 32.0 * N * C, [&]() { return p3d_gn_finalize(a.g2, N, R, a.eps, c.s); });
    }
    launch(c, ka.c_str(), 0, tens * io, [&]() { return p3d_gn_apply(a, c.s); });
}
void gn_pass_backward(const Ctx& c, const GnApplyArgs& a, bool small) {
    const double tens = (double)a.M * a.C * 4.0;
    const int R = a.R, C = a.C, N = (int)(a.M / a.R);
    if (small) {
        const std::string ksb = "gn_small_bwd_kernel<" + std::to_string(a.mode) + ">";
        launch(c, ksb.c_str(), 0, tens * (a.y2 ? 5 : 3), [&]() { return p3d_gn_small_bwd(a, c.s); });
        return;
    }
    const std::string kr = "gn_bwd_reduce_kernel<" + std::to_string(a.mode) + ">";
    const std::string kb = "gn_bwd_apply_kernel<" + std::to_string(a.mode) + ">";
    launch(c, kr.c_str(), 0, tens * (a.y2 ? 3 : 2), [&]() { return p3d_gn_bwd_reduce(a, c.s); });
    launch(c, "gn_bwd_finalize_kernel", 0, 64.0 * N * C, [&]() { return p3d_gn_bwd_finalize(a.g1, N, R, a.dgamma1, a.dbeta1, c.s); });
    if (a.mode == 3)
        launch(c, "gn_bwd_finalize_kernel", 0, 64.0 * N * C, [&]() { return p3d_gn_bwd_finalize(a.g2, N, R, a.dgamma2, a.dbeta2, c.s); });
    launch(c, kb.c_str(), 0, tens * (a.y2 ? 5 : 3), [&]() { return p3d_gn_bwd_apply(a, c.s); });
}

// A BatchNorm's parameters, moving statistics, [4][C] table of scale, shift, mean, invstd, and the statistics partials.
BnParams bn_layout(const float* gamma, const float* beta, float* moving_mean, float* moving_var, float* tab, const float* statpart,
                   int nparts, int C) {
    BnParams b;
    b.gamma = gamma; b.beta = beta; b.moving_mean = moving_mean; b.moving_var = moving_var; b.statpart = statpart; b.nparts = nparts;
    b.scale = tab; b.shift = tab + C; b.mean = tab + 2 * C; b.invstd = tab + 3 * C; b.C = C;
    return b;
}

// One BatchNorm normalise / ReLU / add pass (bn_apply in net_ops.inc, and the test hook p3d_debug_bn_pass).  Index 1 of the
// per-BatchNorm arrays is the second BatchNorm of modes 2 and 3; the kernels' argument structs are built from this, and only here.
struct BnPass {
    int mode = 0; int64_t M = 0; int C = 0;
    const float* y1 = nullptr; int ld1 = 0; const float* y2 = nullptr; int ld2 = 0;
    float* z = nullptr; int ldz = 0; const float* dz = nullptr; int lddz = 0;
    float* dy1 = nullptr; int lddy1 = 0; float* dy2 = nullptr; int lddy2 = 0; int acc2 = 0;
    BnParams bn[2] = {};
    float* dgamma[2] = {}; float* dbeta[2] = {};
    float* part[2] = {}; int nparts = 0; float* coef[2] = {};      // backward partial sums [nparts][C][2] and coefficients [C][2]
    int batch[2] = {};                                              // 1: batch statistics, 0: moving statistics
    float drop_rate = 0.f, drop_scale = 0.f; unsigned long long seed = 0; const unsigned long long* seed_dev = nullptr;
    float eps = 1e-3f;
};
BnApplyArgs bn_apply_args(const BnPass& p) {
    BnApplyArgs a;
    memset(&a, 0, sizeof(a));
    a.mode = p.mode; a.M = p.M; a.C = p.C;
    a.y1 = p.y1; a.ld1 = p.ld1; a.scale1 = p.bn[0].scale; a.shift1 = p.bn[0].shift;
    a.y2 = p.y2; a.ld2 = p.ld2; a.scale2 = p.bn[1].scale; a.shift2 = p.bn[1].shift;
    a.z = p.z; a.ldz = p.ldz;
    a.drop_scale = p.drop_scale; a.drop_rate = p.drop_rate; a.seed = p.seed; a.seed_dev = p.seed_dev;
    return a;
}
BnSmallArgs bn_small_args(const BnPass& p, bool update_moving) {
    BnSmallArgs a;
    memset(&a, 0, sizeof(a));
    a.mode = p.mode; a.M = (int)p.M; a.C = p.C;
    a.y1 = p.y1; a.ld1 = p.ld1; a.y2 = p.y2; a.ld2 = p.ld2;
    a.bn1 = p.bn[0]; a.bn2 = p.bn[1]; a.batch1 = p.batch[0]; a.batch2 = p.batch[1];
    a.update_moving = update_moving; a.eps = p.eps;
    a.z = p.z; a.ldz = p.ldz; a.dz = p.dz; a.lddz = p.lddz;
    a.dy1 = p.dy1; a.lddy1 = p.lddy1; a.dy2 = p.dy2; a.lddy2 = p.lddy2; a.acc2 = p.acc2;
    a.dgamma1 = p.dgamma[0]; a.dbeta1 = p.dbeta[0]; a.dgamma2 = p.dgamma[1]; a.dbeta2 = p.dbeta[1];
    return a;
}
BnBwdArgs bn_bwd_args(const BnPass& p) {
    BnBwdArgs a;
    memset(&a, 0, sizeof(a));
    a.mode = p.mode; a.M = p.M; a.C = p.C; a.dz = p.dz; a.lddz = p.lddz;
    a.y1 = p.y1; a.ld1 = p.ld1; a.scale1 = p.bn[0].scale; a.shift1 = p.bn[0].shift; a.mean1 = p.bn[0].mean; a.invstd1 = p.bn[0].invstd;
    a.y2 = p.y2; a.ld2 = p.ld2; a.scale2 = p.bn[1].scale; a.shift2 = p.bn[1].shift; a.mean2 = p.bn[1].mean; a.invstd2 = p.bn[1].invstd;
    a.gamma1 = p.bn[0].gamma; a.gamma2 = p.bn[1].gamma;
    a.part1 = p.part[0]; a.part2 = p.part[1]; a.nparts = p.nparts; a.coef1 = p.coef[0]; a.coef2 = p.coef[1];
    a.dgamma1 = p.dgamma[0]; a.dbeta1 = p.dbeta[0]; a.dgamma2 = p.dgamma[1]; a.dbeta2 = p.dbeta[1];
    a.batch1 = p.batch[0]; a.batch2 = p.batch[1];
    a.dy1 = p.dy1; a.lddy1 = p.lddy1; a.dy2 = p.dy2; a.lddy2 = p.lddy2; a.acc2 = p.acc2;
    a.drop_scale = p.drop_scale; a.drop_rate = p.drop_rate; a.seed = p.seed; a.seed_dev = p.seed_dev;
    return a;
}

// Which kernels take a BatchNorm pass: the one-launch small-tensor kernels unless the pass drops out; else finalize + apply in
// one launch when every apply block can fold its own channels' statistics partials (nparts of the batch-statistics BatchNorms,
// 0 for the others); else finalize, then apply.  The network makes the small-path choice when it builds the graph (a producer
// whose output takes it writes no statistics partials: stats_target), and its dry runs take finalize + apply.
enum BnPath { BN_SMALL = 1, BN_FOLD = 2, BN_FINALIZE = 3 };      // (p3d_debug_bn_pass's path numbers)
BnPath bn_path(int64_t M, int C, bool dropout, int nparts1, int nparts2, float drop_scale) {
    if (!dropout && p3d_bn_small_ok((long)M, C)) return BN_SMALL;
    return p3d_bn_fold_apply_ok((long)M, C, nparts1, nparts2, drop_scale) ? BN_FOLD : BN_FINALIZE;
}
void bn_pass_forward(const Ctx& c, const BnPass& p, BnPath path, bool update_moving) {
    const double io = (double)p.M * p.C * 4.0 * (p.y2 ? 3 : 2);
    const std::string m = "<" + std::to_string(p.mode) + ">";
    if (path == BN_SMALL) {
        const BnSmallArgs a = bn_small_args(p, update_moving);
        launch(c, ("bn_small_fwd_kernel" + m).c_str(), 0, io, [&]() { return p3d_bn_small_fwd(a, c.s); });
        return;
    }
    const BnApplyArgs a = bn_apply_args(p);
    if (path == BN_FOLD) {
        launch(c, "bn_fold_apply_kernel", 0, io, [&]() {
            return p3d_bn_fold_apply(a, p.bn[0], p.bn[1], p.batch[0], p.batch[1], update_moving ? 1 : 0, p.eps, c.s);
        });
        return;
    }
    for (int q = 0; q < (p.mode == 2 || p.mode == 3 ? 2 : 1); ++q)
        launch(c, "bn_finalize_kernel", 0, 64.0 * p.C, [&]() {
            return p3d_bn_finalize(p.bn[q], p.M, p.batch[q], p.batch[q] && update_moving, p.eps, c.s);
        });
    launch(c, ("bn_apply_kernel" + m).c_str(), 0, io, [&]() { return p3d_bn_apply(a, c.s); });
}
// stem non-null: the pass ends before its apply launch and leaves that launch's arguments there (the stem conv's filter
// gradient evaluates it on its operand path, stem_wgrad.hip).
void bn_pass_backward(const Ctx& c, const BnPass& p, bool small, BnBwdArgs* stem = nullptr) {
    const double tens = (double)p.M * p.C * 4.0;
    const std::string m = "<" + std::to_string(p.mode) + ">";
    if (small) {
        const BnSmallArgs a = bn_small_args(p, false);
        launch(c, ("bn_small_bwd_kernel" + m).c_str(), 0, tens * (p.y2 ? 5 : 3), [&]() { return p3d_bn_small_bwd(a, c.s); });
        return;
    }
    const BnBwdArgs a = bn_bwd_args(p);
    launch(c, ("bn_bwd_reduce_kernel" + m).c_str(), 0, tens * (p.y2 ? 3 : 2), [&]() { return p3d_bn_bwd_reduce(a, c.s); });
    launch(c, "bn_bwd_finalize_kernel", 0, 64.0 * p.C, [&]() { return p3d_bn_bwd_finalize(a, c.s); });
    if (stem) { *stem = a; return; }
    launch(c, ("bn_bwd_apply_kernel" + m).c_str(), 0, tens * (p.y2 ? 5 : 3), [&]() { return p3d_bn_bwd_apply(a, c.s); });
}

// CBAM (cbam() in net_gn.inc, and the test hook p3d_debug_cbam): row chunks per sample of the pooling and backward passes, and the
// layout of a site's scratch, in floats from its base: part [N][chunks][C][3]; avg, mx, ties, cs, davg, dmx [N][C] each;
// havg, hmx, dh [N][C/8], [N][C/8], [N][2][C/8] (+ 8); sp [M][2]; ss [M]; dpre [M]; dsp [M][2]; dcs_part [N][chunks][C]; dO [N][C].
int cbam_chunks(int R) {
    int chunks = R / 16;
    if (chunks < 1) chunks = 1;
    if (chunks > 64) chunks = 64;
    return chunks;
}
struct CbamLayout { int64_t vec, cs, h, sp, ss, dpre, dsp, dcs, dO, total; };
CbamLayout cbam_layout(int64_t N, int64_t M, int64_t C, int64_t chunks) {
    CbamLayout L;
    const int64_t nc = N * C;
    L.vec = nc * chunks * 3;
    L.cs = L.vec + 3 * nc;
    L.h = L.vec + 6 * nc;
    L.sp = L.h + 4 * N * (C / 8) + 8;
    L.ss = L.sp + 2 * M;
    L.dpre = L.ss + M;
    L.dsp = L.dpre + M;
    L.dcs = L.dsp + 2 * M;
    L.dO = L.dcs + nc * chunks;
    L.total = ((L.dO + nc + 63) / 64) * 64;
    return L;
}
// the scratch pointers of CbamArgs for a site whose scratch starts at b (a.N, a.C, a.Ch and a.chunks already set)
void cbam_scratch_args(CbamArgs& a, float* b, int64_t M) {
    const CbamLayout L = cbam_layout(a.N, M, a.C, a.chunks);
    const int64_t nc = (int64_t)a.N * a.C;
    a.part = b;
    float* v = b + L.vec;
    a.avg = v; a.mx = v + nc; a.ties = v + 2 * nc; a.cs = v + 3 * nc; a.davg = v + 4 * nc; a.dmx = v + 5 * nc;
    a.havg = b + L.h; a.hmx = a.havg + (int64_t)a.N * a.Ch; a.dh = a.hmx + (int64_t)a.N * a.Ch;
    a.sp = b + L.sp; a.ss = b + L.ss; a.dpre = b + L.dpre; a.dsp = b + L.dsp;
    a.dcs_part = b + L.dcs;
    a.dO = b + L.dO;
}

// CbamArgs on raw pointers (x and dx: rows of ld floats; w, dw: k0, b0, k1, b1, k7 and their gradients), and the two launches.
CbamArgs cbam_args(int N, int D, int H, int W, int C, const float* x, int ld, const float* const w[5], int chunks, float* scratch,
                   const float* dout, float* dx, int accx, float* const dw[5]) {
    CbamArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.ld = ld; a.N = N; a.D = D; a.H = H; a.W = W; a.C = C; a.Ch = C / 8;
    a.k0 = w[0]; a.b0 = w[1]; a.k1 = w[2]; a.b1 = w[3]; a.k7 = w[4];
    a.chunks = chunks; a.dout = dout; a.dx = dx; a.lddx = ld; a.accx = accx;
    cbam_scratch_args(a, scratch, (int64_t)N * D * H * W);
    a.dk0 = dw[0]; a.db0 = dw[1]; a.dk1 = dw[2]; a.db1 = dw[3]; a.dk7 = dw[4];
    return a;
}
double cbam_elems(const CbamArgs& a) { return (double)a.N * a.D * a.H * a.W * a.C; }
void cbam_pass_forward(const Ctx& c, const CbamArgs& a) { launch(c, "cbam_forward(5 kernels)", 0, 8.0 * cbam_elems(a), [&]() { return p3d_cbam_forward(a, c.s); }); }
void cbam_pass_backward(const Ctx& c, const CbamArgs& a) { launch(c, "cbam_backward(6 kernels)", 0, 28.0 * cbam_elems(a), [&]() { return p3d_cbam_backward(a, c.s); }); }

// Runs `f(side_ctx)` on the side stream after everything queued so far on the main stream.
template <typename F>
void on_side_stream(const Ctx& c, hipEvent_t ev, F&& f) {
    if (c.dry || !c.side || !ev) { f(c); return; }
    // timing diagnostic (WRONG RESULTS): P3D_TUNE_SKIP_SIDE=deconv,block1 drops the side-stream jobs queued during the backward of
    // ops whose name contains one of the substrings -- what that share of the filter gradients costs the step
    static const char* skip = [] {
        const char* e = p3d_tune_env("P3D_TUNE_SKIP_SIDE");
        if (e) fprintf(stderr, "[p3d] P3D_TUNE_SKIP_SIDE=%s: filter gradients are being DROPPED -- timing diagnostic, every result of this process is wrong\n", e);
        return e;
    }();
    if (skip && c.bwd_op) {
        std::string pats(skip), name(c.bwd_op);
        size_t a = 0;
        while (a <= pats.size()) {
            size_t b = pats.find(',', a);
            if (b == std::string::npos) b = pats.size();
            if (b > a && name.find(pats.substr(a, b - a)) != std::string::npos) return;
            a = b + 1;
        }
    }
    if (c.defer) { c.defer->emplace_back(ev, std::function<void(const Ctx&)>(f)); return; }   // f must own what it names
    HIPCHECK(ev_record(ev, c.s));
    HIPCHECK(ev_wait(c.side, ev));
    Ctx sc = c;
    sc.s = c.side;
    f(sc);
}

void wgrad_work(const WgradArgs& a, double& flops, double& bytes) {
    const double M = (double)a.N * a.Gd * a.Gh * a.Gw;
    const double side = (double)a.N * a.Di * a.Hi * a.Wi;
    flops = 2.0 * M * a.ntaps * (double)a.K * a.Nc;
    bytes = 4.0 * (std::min(M * a.ntaps, side) * a.K + M * a.Nc + (double)a.ntaps * a.K * a.Nc);
}

void launch_wgrad(const Ctx& c, const WgradArgs& a0) {
    WgradArgs a = a0;
    double fl, by;
    wgrad_work(a, fl, by);
    a.zeros = g_zero_page;
    launch(c, p3d_wgrad2_variant(a), fl, by, [&]() { return p3d_launch_wgrad2(a, c.s); });
}

// One grouped filter-gradient launch of up to P3D_WGRAD_GROUP problems (conv_wgrad2.hip; flush_wgrads, and the test hook
// p3d_debug_wgrad_group): the label it goes out under, and the launch on c.s with the summed work `fl` / `by` of its members.
const char* wgrad_group_name(const std::vector<WgradArgs>& probs) {
    bool any_fused = false;
    for (auto& pr : probs) any_fused |= pr.xt != 0 || pr.dyt != 0;
    return p3d_wgrad2_group_variant(probs.data(), (int)probs.size(), any_fused);
}
void launch_wgrad_group(const Ctx& c, const std::vector<WgradArgs>& probs, const char* name, double fl, double by) {
    launch(c, name, fl, by, [&]() { return p3d_launch_wgrad2_group(probs.data(), (int)probs.size(), c.s); });
}

// ---- BatchNorm fused into the convs' operand paths: the launches, on plain descriptors ------------------------------------------
// conv() (net_ops.inc) and the test hooks p3d_debug_fused_conv / p3d_debug_fused_wgrad build their fused launches with these:
// device pointers, row strides, channel counts, partial pointers and counts, rows and publish / update-moving flags in; the
// fields of IgemmArgs / WgradArgs (and the finalize launches) out.  Nothing here knows an Act or a BN.
struct FusedBn {               // forward: the BatchNorm of one source of a RELU1 / RELU2 operand
    const float* gamma = nullptr; const float* beta = nullptr; int C = 0;
    float *scale = nullptr, *shift = nullptr, *mean = nullptr, *invstd = nullptr;      // the published values
    float *moving_mean = nullptr, *moving_var = nullptr;
    const float* part = nullptr; int nparts = 0;      // the producer's (sum, sumsq) partials [nparts][C][2]
    int64_t rows = 0;                                 // rows of the normalised tensor
    int pub = 0;                                      // 0: read the published scale / shift, 1: fold the partials and publish, 2: fold only
    bool update_moving = false;
};
struct FusedBnGrad {           // backward: the BatchNorm a GRAD operand / a dyt filter gradient differentiates through
    const float* gamma = nullptr; const float* mean = nullptr; const float* invstd = nullptr; int C = 0;
    float *coef = nullptr, *dgamma = nullptr, *dbeta = nullptr;      // published k1 / k2 / k3 [3][C] and the parameter gradients
    const float* part = nullptr; int nparts = 0;      // the gating launch's (sum g, sum g*xhat) partials [nparts][C][2]
    int64_t rows = 0;
};
// THE rule: up to P3D_FOLD_MAX partials a consuming launch folds in its own prologue; more go through a finalize launch, and
// every consumer then reads the published values.
inline bool fused_needs_finalize(int nparts) { return nparts > P3D_FOLD_MAX; }
// forward: the finalize launch of a publishing source with many partials; true when it went out (the values are then complete)
bool fused_bn_prefinalize(const Ctx& c, const FusedBn& d) {
    if (d.pub != 1 || !fused_needs_finalize(d.nparts)) return false;
    BnParams bp;
    memset(&bp, 0, sizeof(bp));
    bp.gamma = d.gamma; bp.beta = d.beta; bp.moving_mean = d.moving_mean; bp.moving_var = d.moving_var;
    bp.statpart = d.part; bp.nparts = d.nparts; bp.scale = d.scale; bp.shift = d.shift; bp.mean = d.mean; bp.invstd = d.invstd; bp.C = d.C;
    launch(c, "bn_finalize_kernel", 0, 64.0 * d.C, [&]() { return p3d_bn_finalize(bp, (long)d.rows, 1, d.update_moving ? 1 : 0, 1e-3f, c.s); });
    return true;
}
BnFold fused_bn_fold(const FusedBn& d, bool finalized) {
    BnFold f;
    memset(&f, 0, sizeof(f));
    f.gamma = d.gamma; f.beta = d.beta; f.C = d.C;
    f.scale = d.scale; f.shift = d.shift; f.mean = d.mean; f.invstd = d.invstd;
    f.moving_mean = d.moving_mean; f.moving_var = d.moving_var;
    f.inv_m = 1.0 / (double)d.rows; f.eps = 1e-3f;
    const bool fold = d.pub != 0 && !finalized;
    if (fold) { f.part = d.part; f.nparts = d.nparts; }
    f.publish = (fold && d.pub == 1) ? 1 : 0;
    f.update_moving = d.update_moving ? 1 : 0;
    return f;
}
// RELU1 / RELU2 on a forward launch whose gathered operand `a.x` is the raw tensor of source 0; y2 / ld2: the raw tensor of source 1
void fused_forward_operand(IgemmArgs& a, int at, const FusedBn& s1, bool fin1, const float* y2, int ld2, const FusedBn* s2, bool fin2) {
    if (at != P3D_AT_RELU1 && at != P3D_AT_RELU2) throw P3dError("a fused forward operand is RELU1 or RELU2");
    a.at_mode = at;
    a.f1 = fused_bn_fold(s1, fin1);
    if (at == P3D_AT_RELU2) {
        if (!s2) throw P3dError("RELU2 needs its second source");
        a.x2 = y2; a.ldx2 = ld2; a.f2 = fused_bn_fold(*s2, fin2);
    }
}
BnGradFold fused_bn_grad_fold(const FusedBnGrad& d, bool finalized, bool publish) {
    BnGradFold f;
    memset(&f, 0, sizeof(f));
    f.gamma = d.gamma; f.mean = d.mean; f.invstd = d.invstd; f.C = d.C;
    f.coef = d.coef; f.dgamma = d.dgamma; f.dbeta = d.dbeta;
    f.inv_m = 1.0 / (double)d.rows;
    const bool fold = !finalized;
    if (fold) { f.part = d.part; f.nparts = d.nparts; }
    f.publish = (fold && publish) ? 1 : 0;
    return f;
}
// backward: the finalize launch for many gradient partials; true when it went out
bool fused_bn_grad_prefinalize(const Ctx& c, const FusedBnGrad& d) {
    if (!fused_needs_finalize(d.nparts)) return false;
    const BnGradFold gf = fused_bn_grad_fold(d, false, true);
    launch(c, "bn_grad_finalize_kernel", 0, 64.0 * d.C, [&]() { return p3d_bn_grad_finalize(gf, c.s); });
    return true;
}
// GRAD on an input-gradient launch whose gathered operand `a.x` is the gated gradient; y / ldy: the BatchNorm's input there
void fused_grad_operand(IgemmArgs& a, const float* y, int ldy, const FusedBnGrad& d, bool finalized, bool publish) {
    a.at_mode = P3D_AT_GRAD; a.x2 = y; a.ldx2 = ldy;
    a.gf = fused_bn_grad_fold(d, finalized, publish);
}
// the gated epilogue belongs to stride-1 convs whose input gradient is ONE launch
void fused_gate_check(const int s[3], int ngate) {
    if (ngate && (s[0] != 1 || s[1] != 1 || s[2] != 1)) throw P3dError("gated input gradients need a stride-1 conv");
}
// ngate gates on the launches `v` of an input gradient; returns the rows of (sum g, sum g*xhat) partials every gate gets (one per
// output-tile row of the launch's plan; 0 when `plan_rows` is off -- a planning pass)
int fused_gated_epilogue(std::vector<IgemmArgs>& v, int ngate, const BnGate* gate, bool raw_store, bool plan_rows) {
    if (ngate < 1 || ngate > 2) throw P3dError("a gated epilogue has one or two gates");
    if (v.size() != 1) throw P3dError("gated input gradient with more than one residue class");
    IgemmArgs& a = v[0];
    a.ngate = ngate; a.raw_store = raw_store ? 1 : 0;
    for (int q = 0; q < ngate; ++q) a.gate[q] = gate[q];
    if (!plan_rows) return 0;
    IgemmArgs t = a; t.zeros = g_zero_page;
    return p3d_igemm2_mtiles(t, p3d_igemm2_plan(t, 1));
}
// filter gradients: relu(scale*y + shift) (one or two sources) on the gathered side, k1*g + k2*y + k3 on the dense side
void fused_wgrad_x(WgradArgs& wa, int xt, const float* xs1, const float* xt1, const float* x2, int ldx2, const float* xs2, const float* xt2) {
    if (xt != 1 && xt != 2) throw P3dError("a fused filter-gradient operand has one or two sources");
    wa.xt = xt; wa.xs1 = xs1; wa.xt1 = xt1;
    if (xt == 2) { wa.x2 = x2; wa.ldx2 = ldx2; wa.xs2 = xs2; wa.xt2 = xt2; }
}
void fused_wgrad_dy(WgradArgs& wa, const float* y, int ldy, const float* coef) { wa.dyt = 1; wa.dy2 = y; wa.ldy2 = ldy; wa.dcoef = coef; }

struct Op {
    std::string name, kind;
    double flops = 0, bytes = 0;            // forward algorithmic work
    double bflops = 0, bbytes = 0;          // backward algorithmic work
    std::vector<struct Param*> owns;        // trainable variables whose gradients this op's backward produces
    std::function<void(const Ctx&)> fwd, bwd;
    // Decisions of the last forward, for the decision-pinned parity tests (p3d_debug_decision_*): a normalise / ReLU pass runs
    // its OWN backward kernel on dz = 1 with the statistics terms off (the inference form dy = gamma*invstd * gate), so what
    // comes out is non-zero exactly where the gate of the real backward is open; a max-pool hands out its input.
    std::string dec_kind;                   // "" (none), "bn", "pool"
    std::string dec_name1, dec_name2;       // bn: TF scopes of the one or two BatchNorms
    const struct Act* dec_act = nullptr;    // bn: shape of the gated tensor; pool: the pool's input
    int64_t dec_scratch = 0;                // floats of scratch the gates closure needs (0: 4 x channels)
    std::function<void(hipStream_t, const float* ones, float* o1, float* o2, float* scratch)> gates;
};

struct ConvGeo {       // a SAME forward conv: input extents -> output extents
    int k[3], s[3], pad[3], I[3], O[3];
};

ConvGeo make_geo(int Di, int Hi, int Wi, const int k[3], const int s[3]) {
    ConvGeo g;
    const int in[3] = {Di, Hi, Wi};
    for (int a = 0; a < 3; ++a) {
        g.k[a] = k[a]; g.s[a] = s[a]; g.I[a] = in[a];
        g.O[a] = (in[a] + s[a] - 1) / s[a];
        int pt = (g.O[a] - 1) * s[a] + k[a] - in[a];
        if (pt < 0) pt = 0;
        g.pad[a] = pt / 2;
    }
    return g;
}

// tf.nn.max_pool3d SAME over an [N, g.I, C] tensor with row strides ldx / ldy (input / output, and their gradients): all of
// PoolArgs but the pointers
PoolArgs pool_args(const ConvGeo& g, int N, int C, int ldx, int ldy) {
    PoolArgs a;
    memset(&a, 0, sizeof(a));
    a.N = N; a.Di = g.I[0]; a.Hi = g.I[1]; a.Wi = g.I[2]; a.C = C; a.ldx = a.lddx = ldx;
    a.Do = g.O[0]; a.Ho = g.O[1]; a.Wo = g.O[2]; a.ldy = a.lddy = ldy;
    a.kd = g.k[0]; a.kh = g.k[1]; a.kw = g.k[2]; a.sd = g.s[0]; a.sh = g.s[1]; a.sw = g.s[2];
    a.pd = g.pad[0]; a.ph = g.pad[1]; a.pw = g.pad[2];
    return a;
}

// The pool's launches (maxpool() in net_ops.inc, and the max_pool3d entry points).  The backward reads the forward's output (disjoint
// windows: the first cell equal to the maximum) or its arg-max table (overlapping windows: a gather); returns the kernel it launched.
double pool_bytes(const PoolArgs& a) { return 4.0 * ((int64_t)a.N * a.Di * a.Hi * a.Wi + (int64_t)a.N * a.Do * a.Ho * a.Wo) * a.C; }
void pool_forward(const Ctx& c, const PoolArgs& a) { launch(c, "maxpool_fwd_kernel", 0, pool_bytes(a), [&]() { return p3d_maxpool_fwd(a, c.s); }); }
const char* pool_backward(const Ctx& c, const PoolArgs& a, int accumulate) {
    if (p3d_maxpool_disjoint(a)) {
        launch(c, "maxpool_bwd_disjoint_kernel", 0, pool_bytes(a) * 2, [&]() { return p3d_maxpool_bwd_disjoint(a, accumulate, c.s); });
        return "maxpool_bwd_disjoint_kernel";
    }
    if (!a.idx) throw P3dError("max-pool with overlapping windows was built without its arg-max table");
    launch(c, "maxpool_bwd_gather_kernel", 0, pool_bytes(a) * 2, [&]() { return p3d_maxpool_bwd_gather(a, accumulate, c.s); });
    return "maxpool_bwd_gather_kernel";
}

// The output head (head() in net_graphs.inc, and the test hook p3d_debug_head): HeadArgs on raw pointers, and the three launches.
// transpose: the stride-2 conv3d_transpose head (p3d_head_*), else the stride-1 conv (p3d_headc_*); path, done: as the launchers'.
HeadArgs head_args(const float* x, int N, int D, int H, int W, int C, const float* k, const float* bias, float* logits, float* pred,
                   int sigmoid, const float* dlogits, float* dx, float* dk, float* dbias) {
    HeadArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.N = N; a.D = D; a.H = H; a.W = W; a.C = C;
    a.k = k; a.bias = bias; a.logits = logits; a.pred = pred; a.sigmoid = sigmoid;
    a.dlogits = dlogits; a.dx = dx; a.dk = dk; a.dbias = dbias;
    return a;
}
LaunchDesc head_desc(const HeadArgs& a, bool transpose, const char* kernel, const char* kernel_stride1) {
    const int64_t rows = (int64_t)a.N * a.D * a.H * a.W, out_rows = transpose ? 8 * rows : rows;
    return {transpose ? kernel : kernel_stride1, 2.0 * rows * 27 * a.C, 4.0 * (rows * (double)a.C + 2.0 * out_rows)};
}
void head_forward(const Ctx& c, const HeadArgs& a, bool transpose, int path = P3D_HEAD_RULE, HeadLaunch* done = nullptr) {
    const LaunchDesc d = head_desc(a, transpose, "head_fwd_kernel", "headc_fwd_kernel");
    launch(c, d.kernel, d.flops, d.bytes, [&]() { return transpose ? p3d_head_fwd(a, c.s, path, done) : p3d_headc_fwd(a, c.s, done); });
}
void head_filter_gradient(const Ctx& c, const HeadArgs& a, bool transpose, int path = P3D_HEAD_RULE, HeadLaunch* done = nullptr) {
    const LaunchDesc d = head_desc(a, transpose, "head_bwd_filter_kernel", "headc_bwd_filter_kernel");
    launch(c, d.kernel, d.flops, d.bytes, [&]() { return transpose ? p3d_head_bwd_filter(a, c.s, path, done) : p3d_headc_bwd_filter(a, c.s, done); });
}
void head_input_gradient(const Ctx& c, const HeadArgs& a, bool transpose) {      // (one kernel each: nothing to force or report)
    const LaunchDesc d = head_desc(a, transpose, "head_bwd_input_kernel", "headc_bwd_input_kernel");
    launch(c, d.kernel, d.flops, d.bytes, [&]() { return transpose ? p3d_head_bwd_input(a, c.s) : p3d_headc_bwd_input(a, c.s); });
}

// The attention block's mixing pass (attn_run in net_graphs.inc, and the test hook p3d_debug_attn_mix): AttnMixArgs on raw pointers
// (z / dz, r / dr and x / dx share their row strides), and the launches.
AttnMixArgs attn_mix_args(int64_t M, int C, const float* r, int ldr, const float* x, int ldx, const float* gamma, float* z, int ldz,
                          const float* dz, float* dr, float* dx, int accx, float* dgamma, const Ctx& c, bool dropout) {
    AttnMixArgs a;
    memset(&a, 0, sizeof(a));
    a.M = M; a.C = C; a.r = r; a.ldr = ldr; a.x = x; a.ldx = ldx; a.gamma = gamma;
    a.z = z; a.ldz = ldz; a.dz = dz; a.dr = dr; a.dx = dx; a.accx = accx; a.dgamma = dgamma;
    set_dropout(a, c, dropout);
    return a;
}
void attn_mix_forward(const Ctx& c, const AttnMixArgs& a) { launch(c, "mix_fwd_kernel", 0, 4.0 * 3 * a.M * a.C, [&]() { return p3d_attn_mix_fwd(a, c.s); }); }
void attn_mix_backward(const Ctx& c, const AttnMixArgs& a) { launch(c, "mix_bwd_kernel", 0, 4.0 * 5 * a.M * a.C, [&]() { return p3d_attn_mix_bwd(a, c.s); }); }

inline int pmod(int a, int m) { int r = a % m; return r < 0 ? r + m : r; }

// firstconv1 (p3d.py:172) on its packed form: the clip is copied to 4 channels with the SAME padding of the W axis written out
// (x4 [rows][Wp][4]), so that a kernel ROW is one tap of K = kw*4 contiguous floats (7 taps of K = 28 instead of 49 of K = 3).
// This describes the packed problem -- buffer sizes in floats and the packing launches -- and allocates nothing: the network
// keeps the buffers in its arena, the op entry points in DevBufs.
struct StemGeo {
    ConvGeo g; int N, Cout, Wp, K4, KH; int64_t xrows;
    int64_t x4_floats, w4_floats;      // x4; w4 and the packed filter gradient dw4 [kh][kw*4][Cout]
    int64_t part_floats;               // scratch of the one-pass filter gradient (stem_wgrad.hip); 0: that kernel does not take the shape
};
StemGeo stem_geo(const ConvGeo& g, int N, int Cout) {
    if (g.k[0] != 1) throw P3dError("stem mode needs kd == 1");
    StemGeo sg;
    const int pad_total = std::max((g.O[2] - 1) * g.s[2] + g.k[2] - g.I[2], 0);
    sg.g = g; sg.N = N; sg.Cout = Cout;
    sg.Wp = g.I[2] + pad_total; sg.K4 = g.k[2] * 4; sg.KH = g.k[1];
    sg.xrows = (int64_t)N * g.I[0] * g.I[1];
    sg.x4_floats = sg.xrows * sg.Wp * 4; sg.w4_floats = (int64_t)sg.KH * sg.K4 * Cout;
    sg.part_floats = p3d_stem_wgrad_ok(g.k[0], g.k[1], g.k[2], 3, Cout, g.s[0], g.s[1], g.s[2], g.O[2]) ? p3d_stem_wgrad_part_floats() : 0;
    return sg;
}
// x -> x4 (whose padding columns the owner zeroed once) and, with w, the [kh*kw][3][Cout] filter -> w4
void stem_pack(const Ctx& c, const StemGeo& sg, const float* x, float* x4, const float* w = nullptr, float* w4 = nullptr) {
    const ConvGeo& g = sg.g;
    launch(c, "stem_pad_kernel", 0, 28.0 * (sg.xrows * g.I[2]), [&]() { return p3d_stem_pad(x, x4, sg.xrows, g.I[2], sg.Wp, g.pad[2], c.s); });
    if (w) launch(c, "stem_pack_w_kernel", 0, 8.0 * sg.KH * sg.K4 * sg.Cout, [&]() { return p3d_stem_pack_w(w, w4, sg.KH * g.k[2], sg.Cout, c.s); });
}

// ---- tap tables: the filter taps of a dense SAME conv in [kd][kh][kw] order, and the stem's kernel rows on its packed form;
//      the forward and the filter gradient walk the same list.  Return the tap count.
int conv_taps(const ConvGeo& g, P3dTap* taps) {
    int t = 0;
    for (int kd = 0; kd < g.k[0]; ++kd)
        for (int kh = 0; kh < g.k[1]; ++kh)
            for (int kw = 0; kw < g.k[2]; ++kw) {
                if (t >= P3D_MAX_TAPS) throw P3dError("kernel has too many taps");
                taps[t].dd = (int16_t)(kd - g.pad[0]);
                taps[t].dh = (int16_t)(kh - g.pad[1]);
                taps[t].dw = (int16_t)(kw - g.pad[2]);
                taps[t].widx = (int16_t)((kd * g.k[1] + kh) * g.k[2] + kw);
                ++t;
            }
    return t;
}
int stem_row_taps(const StemGeo& sg, P3dTap* taps) {
    for (int kh = 0; kh < sg.KH; ++kh) { taps[kh].dd = 0; taps[kh].dh = (int16_t)(kh - sg.g.pad[1]); taps[kh].dw = 0; taps[kh].widx = (int16_t)kh; }
    return sg.KH;
}

IgemmArgs stem_forward_args(const StemGeo& sg, const float* x4, const float* w4, float* y, int ldy, const float* bias) {
    const ConvGeo& g = sg.g;
    IgemmArgs a;
    memset(&a, 0, sizeof(a));
    a.N = sg.N; a.Di = g.I[0]; a.Hi = g.I[1]; a.Wi = sg.Wp; a.ldx = 4; a.K = sg.K4;
    a.Gd = g.O[0]; a.Gh = g.O[1]; a.Gw = g.O[2]; a.isd = g.s[0]; a.ish = g.s[1]; a.isw = g.s[2];
    a.ntaps = stem_row_taps(sg, a.taps);
    a.x = x4; a.y = y; a.Do = g.O[0]; a.Ho = g.O[1]; a.Wo = g.O[2]; a.ldy = ldy; a.Nc = sg.Cout;
    a.osd = a.osh = a.osw = 1; a.w = w4; a.bias = bias;
    return a;
}

// ---- launch-argument builders on the shared geometry ---------------------------------------------
IgemmArgs igemm_conv_forward(const ConvGeo& g, int N, const float* x, int ldx, int Cin, float* y, int ldy, int Cout,
                             const float* w, const float* bias, int accum) {
    IgemmArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.N = N; a.Di = g.I[0]; a.Hi = g.I[1]; a.Wi = g.I[2]; a.ldx = ldx; a.K = Cin;
    a.Gd = g.O[0]; a.Gh = g.O[1]; a.Gw = g.O[2];
    a.isd = g.s[0]; a.ish = g.s[1]; a.isw = g.s[2];
    a.y = y; a.Do = g.O[0]; a.Ho = g.O[1]; a.Wo = g.O[2]; a.ldy = ldy; a.Nc = Cout;
    a.osd = a.osh = a.osw = 1;
    a.w = w; a.wT = 0; a.bias = bias; a.accum = accum;
    a.ntaps = conv_taps(g, a.taps);
    return a;
}

// Input-gradient of the conv (== conv3d_transpose forward): one launch per residue class of the
// conv-input lattice.  `dense` has the conv's OUTPUT extents, `out` the conv's INPUT extents.
std::vector<IgemmArgs> igemm_conv_input_side(const ConvGeo& g, int N, const float* dense, int ld_dense, int Cdense,
                                             float* out, int ld_out, int Cout_side, const float* w,
                                             const float* bias, int accum, bool include_empty) {
    std::vector<IgemmArgs> v;
    for (int pd = 0; pd < g.s[0]; ++pd)
        for (int ph = 0; ph < g.s[1]; ++ph)
            for (int pw = 0; pw < g.s[2]; ++pw) {
                const int p[3] = {pd, ph, pw};
                IgemmArgs a;
                memset(&a, 0, sizeof(a));
                bool empty_grid = false;
                int G[3];
                for (int ax = 0; ax < 3; ++ax) {
                    G[ax] = (g.I[ax] - p[ax] + g.s[ax] - 1) / g.s[ax];
                    if (g.I[ax] <= p[ax]) empty_grid = true;
                }
                if (empty_grid) continue;
                a.x = dense; a.N = N; a.Di = g.O[0]; a.Hi = g.O[1]; a.Wi = g.O[2]; a.ldx = ld_dense; a.K = Cdense;
                a.Gd = G[0]; a.Gh = G[1]; a.Gw = G[2];
                a.isd = a.ish = a.isw = 1;
                a.y = out; a.Do = g.I[0]; a.Ho = g.I[1]; a.Wo = g.I[2]; a.ldy = ld_out; a.Nc = Cout_side;
                a.osd = g.s[0]; a.osh = g.s[1]; a.osw = g.s[2];
                a.ood = pd; a.ooh = ph; a.oow = pw;
                a.w = w; a.wT = 1; a.bias = bias; a.accum = accum;
                int t = 0;
                for (int kd = 0; kd < g.k[0]; ++kd) {
                    if (pmod(pd + g.pad[0] - kd, g.s[0])) continue;
                    for (int kh = 0; kh < g.k[1]; ++kh) {
                        if (pmod(ph + g.pad[1] - kh, g.s[1])) continue;
                        for (int kw = 0; kw < g.k[2]; ++kw) {
                            if (pmod(pw + g.pad[2] - kw, g.s[2])) continue;
                            if (t >= P3D_MAX_TAPS) throw P3dError("kernel has too many taps");
                            // exact division (the residue is 0): floor semantics for negatives
                            a.taps[t].dd = (int16_t)((pd + g.pad[0] - kd) / g.s[0]);
                            a.taps[t].dh = (int16_t)((ph + g.pad[1] - kh) / g.s[1]);
                            a.taps[t].dw = (int16_t)((pw + g.pad[2] - kw) / g.s[2]);
                            a.taps[t].widx = (int16_t)((kd * g.k[1] + kh) * g.k[2] + kw);
                            ++t;
                        }
                    }
                }
                a.ntaps = t;
                if (t == 0 && !include_empty) continue;
                v.push_back(a);
            }
    return v;
}

// Filter gradient of the [1,kh,kw,3,Cout] stem conv on its packed form (conv(): "stem"): x4 is the 4-channel, W-padded copy
// of the clip ([rows][Wp][4]), dw4 the packed gradient [kh][kw*4][Cout] (zeroed here); dw += its three real channels.
void stem_filter_gradient(const Ctx& c, const StemGeo& sg, const float* x4, const float* dy, int ldy, float* dw4, float* dw, float* dbias,
                          bool greedy, float* onepass_part = nullptr, const BnBwdArgs* through_bn = nullptr) {
    const ConvGeo& g = sg.g;
    const int N = sg.N, Wp = sg.Wp, Cout = sg.Cout, KH = sg.KH, K4 = sg.K4;
    if (onepass_part && !dbias && sg.part_floats) {
        // one pass over the output gradient (stem_wgrad.hip); through_bn: that gradient is the BatchNorm + ReLU OUTPUT's and
        // the normalisation's backward apply pass runs on this kernel's operand path
        StemWgradArgs a;
        memset(&a, 0, sizeof(a));
        a.x4 = x4; a.Wp = Wp; a.Hi = g.I[1]; a.nimg = N * g.I[0]; a.Ho = g.O[1]; a.Wo = g.O[2]; a.pad_h = g.pad[1];
        a.dy = dy; a.lddy = ldy; a.part = onepass_part; a.dw = dw;
        if (through_bn) {
            const BnBwdArgs& b = *through_bn;
            a.fused = 1; a.dy = b.dz; a.lddy = b.lddz; a.y = b.y1; a.ldy = b.ld1;
            a.scale = b.scale1; a.shift = b.shift1; a.mean = b.mean1; a.invstd = b.invstd1; a.gamma = b.gamma1; a.coef = b.coef1; a.batch = b.batch1;
        }
        const double rows = (double)a.nimg * a.Ho * a.Wo;
        int nblocks = 1;
        launch(c, through_bn ? "stem_wgrad_kernel<bn>" : "stem_wgrad_kernel", 2.0 * rows * KH * g.k[2] * 3 * Cout,
               4.0 * rows * Cout * (through_bn ? 2 : 1), [&]() { return p3d_stem_wgrad(a, &nblocks, c.s); });
        launch(c, "stem_wgrad_fold_kernel", 0, 4.0 * nblocks * KH * g.k[2] * 3 * Cout,
               [&]() { return p3d_stem_wgrad_fold(onepass_part, nblocks, dw, c.s); });
        return;
    }
    if (through_bn) throw P3dError("the stem's fused normalisation backward needs the one-pass filter gradient");
    if (!c.dry) HIPCHECK(hipMemsetAsync(dw4, 0, (size_t)KH * K4 * Cout * sizeof(float), c.s));
    WgradArgs wa;
    memset(&wa, 0, sizeof(wa));
    wa.x = x4; wa.N = N; wa.Di = g.I[0]; wa.Hi = g.I[1]; wa.Wi = Wp; wa.ldx = 4; wa.K = K4;
    wa.Gd = g.O[0]; wa.Gh = g.O[1]; wa.Gw = g.O[2]; wa.isd = g.s[0]; wa.ish = g.s[1]; wa.isw = g.s[2];
    wa.dy = dy; wa.ldy = ldy; wa.Nc = Cout; wa.dw = dw4; wa.dbias = dbias; wa.ksplit = 1;
    wa.ntaps = stem_row_taps(sg, wa.taps);
    wa.greedy = greedy ? 1 : 0;
    wa.pair = K4 <= 32 ? 1 : 0;            // 28 floats per kernel row: two rows of the 7x7 kernel per 64-row tile
    launch_wgrad(c, wa);
    launch(c, "stem_unpack_dw_kernel", 0, 8.0 * KH * K4 * Cout, [&]() { return p3d_stem_unpack_dw(dw4, dw, KH * g.k[2], Cout, c.s); });
}

WgradArgs wgrad_conv(const ConvGeo& g, int N, const float* x, int ldx, int Cin, const float* dy, int ldy, int Cout,
                     float* dw, float* dbias) {
    WgradArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.N = N; a.Di = g.I[0]; a.Hi = g.I[1]; a.Wi = g.I[2]; a.ldx = ldx; a.K = Cin;
    a.Gd = g.O[0]; a.Gh = g.O[1]; a.Gw = g.O[2];
    a.isd = g.s[0]; a.ish = g.s[1]; a.isw = g.s[2];
    a.dy = dy; a.ldy = ldy; a.Nc = Cout; a.dw = dw; a.dbias = dbias; a.ksplit = 1;
    a.ntaps = conv_taps(g, a.taps);
    return a;
}

// A plain row-major GEMM  Y[M x Nc] = X[M x K] * W  as a 1x1x1 convolution over one clip's lattice (D,H,W),
// M = D*H*W (the kernels pack lattice coordinates, so M is passed as the lattice it came from).
// W is [K][Nc] (wT = 0) or [Nc][K] (wT = 1), dense.
IgemmArgs gemm_rows(int D, int H, int W, const float* x, int ldx, int K, const float* w, int wT, float* y, int ldy, int Nc) {
    IgemmArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.N = 1; a.Di = D; a.Hi = H; a.Wi = W; a.ldx = ldx; a.K = K;
    a.Gd = D; a.Gh = H; a.Gw = W; a.isd = a.ish = a.isw = 1;
    a.y = y; a.Do = D; a.Ho = H; a.Wo = W; a.ldy = ldy; a.Nc = Nc; a.osd = a.osh = a.osw = 1;
    a.w = w; a.wT = wT;
    a.ntaps = 1;
    return a;
}
// dW[K x Nc] += X[M x K]^T * dY[M x Nc]  on the weight-gradient kernel (dW must be zero before)
WgradArgs gemm_tn(int D, int H, int W, const float* x, int ldx, int K, const float* dy, int ldy, int Nc, float* dw) {
    WgradArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.N = 1; a.Di = D; a.Hi = H; a.Wi = W; a.ldx = ldx; a.K = K;
    a.Gd = D; a.Gh = H; a.Gw = W; a.isd = a.ish = a.isw = 1;
    a.dy = dy; a.ldy = ldy; a.Nc = Nc; a.dw = dw; a.ksplit = 1;
    a.ntaps = 1;
    return a;
}

void zero_strided(const Ctx& c, float* p, int ld, int64_t rows, int C) {
    if (c.dry) {
        if (ld == C) c.dry->push_back({p, (size_t)rows * C * sizeof(float)});      // dense buffers may move into the arena
        return;
    }
    if ((const char*)p >= c.z0 && (const char*)p < c.z1) return;                    // zeroed with the arena
    if (ld == C) HIPCHECK(hipMemsetAsync(p, 0, (size_t)rows * C * sizeof(float), c.s));
    else HIPCHECK(hipMemset2DAsync(p, (size_t)ld * sizeof(float), 0, (size_t)C * sizeof(float), (size_t)rows, c.s));
}

// The stored-score execution of the attention core  o = softmax(g f^T) h  (utils/network.py:183-185) and of its four gradients:
// three GEMMs per direction and clip around a stored [Ng x Nfp] score matrix, Nfp = Nf rounded up to 4 (key / value rows are
// padded with zero rows first; the softmax masks the padded columns).  Described once, on plain pointers, for the graph op
// (attn_run) and the test hook (p3d_debug_attention_core).  f, h, df, dh are dense ([B][Nf][ch/8], [B][Nf][ch]); g / dg and
// o / d_o are rows of ldg and ldo floats.  sbuf, dsbuf: [B][Ng][Nfp]; the four pad buffers ([B][Nfp][ch/8 or ch]) only when
// Nfp != Nf.  (gD, gH, gW) is the lattice the Ng queries of a clip come from (each extent below 1024: packed coordinates).
struct AttnCore {
    int B = 0, Ng = 0, Nf = 0, ch = 0, gD = 1, gH = 1, gW = 1;
    const float* g = nullptr; int ldg = 0;
    const float* f = nullptr; const float* h = nullptr;
    float* o = nullptr; int ldo = 0;
    const float* d_o = nullptr;
    float *dg = nullptr, *df = nullptr, *dh = nullptr;
    float *sbuf = nullptr, *dsbuf = nullptr, *fpad = nullptr, *hpad = nullptr, *dfpad = nullptr, *dhpad = nullptr;
    int ci() const { return ch / 8; }
    int Nfp() const { return (Nf + 3) / 4 * 4; }
    bool pad() const { return Nfp() != Nf; }
    const float* F() const { return pad() ? fpad : f; }
    const float* H() const { return pad() ? hpad : h; }
    // the four row-major products of clip b: scores = g f^T, o = beta h, d beta = d o h^T, d g = d s f
    enum Product { SCORES = 0, OUT = 1, DBETA = 2, DG = 3 };
    IgemmArgs product(int which, int b) const {
        const int64_t sb = (int64_t)b * Ng * Nfp(), fb = (int64_t)b * Nfp() * ci(), hb = (int64_t)b * Nfp() * ch;
        switch (which) {
            case SCORES: return gemm_rows(gD, gH, gW, g + (int64_t)b * Ng * ldg, ldg, ci(), F() + fb, 1, sbuf + sb, Nfp(), Nfp());
            case OUT: return gemm_rows(gD, gH, gW, sbuf + sb, Nfp(), Nfp(), H() + hb, 0, o + (int64_t)b * Ng * ldo, ldo, ch);
            case DBETA: return gemm_rows(gD, gH, gW, d_o + (int64_t)b * Ng * ldo, ldo, ch, H() + hb, 1, dsbuf + sb, Nfp(), Nfp());
            default: return gemm_rows(gD, gH, gW, dsbuf + sb, Nfp(), Nfp(), F() + fb, 0, dg + (int64_t)b * Ng * ldg, ldg, ci());
        }
    }
    int splits(int which) const { return std::max(1, p3d_igemm2_plan(product(which, 0), 1).splits); }
    // one GEMM per clip; if the planner slices K (few rows), the whole output is zeroed once and the launches add
    void gemm_each(const Ctx& c, int which, float* out, int ld, int Nc) const {
        const bool split = splits(which) > 1;
        if (split) zero_strided(c, out, ld, (int64_t)B * Ng, Nc);
        for (int b = 0; b < B; ++b) launch_igemm(c, product(which, b), split ? 1 : 0);
    }
    void forward(const Ctx& c) const {
        const int Np = Nfp(), k = ci();
        if (pad()) {
            launch(c, "pad_rows_kernel", 0, 8.0 * B * Np * k, [&]() { return p3d_pad_rows(f, fpad, B, Nf, Np, k, c.s); });
            launch(c, "pad_rows_kernel", 0, 8.0 * B * Np * ch, [&]() { return p3d_pad_rows(h, hpad, B, Nf, Np, ch, c.s); });
        }
        gemm_each(c, SCORES, sbuf, Np, Np);
        launch(c, "softmax_fwd_kernel", 0, 8.0 * B * Ng * Np, [&]() { return p3d_softmax_rows(sbuf, (long long)B * Ng, Nf, Np, c.s); });
        gemm_each(c, OUT, o, ldo, ch);
    }
    void backward(const Ctx& c) const {
        const int Np = Nfp(), k = ci();
        float* dF = pad() ? dfpad : df; float* dH = pad() ? dhpad : dh;
        gemm_each(c, DBETA, dsbuf, Np, Np);                                                        // d beta = d o * h^T
        zero_strided(c, dH, ch, (int64_t)B * Np, ch);
        for (int b = 0; b < B; ++b)                                                                // d h = beta^T * d o
            launch_wgrad(c, gemm_tn(gD, gH, gW, sbuf + (int64_t)b * Ng * Np, Np, Np, d_o + (int64_t)b * Ng * ldo, ldo, ch, dH + (int64_t)b * Np * ch));
        launch(c, "softmax_bwd_kernel", 0, 12.0 * B * Ng * Np, [&]() { return p3d_softmax_rows_bwd(sbuf, dsbuf, (long long)B * Ng, Nf, Np, c.s); });
        gemm_each(c, DG, dg, ldg, k);                                                              // d g = d s * f
        zero_strided(c, dF, k, (int64_t)B * Np, k);
        for (int b = 0; b < B; ++b)                                                                // d f = d s^T * g
            launch_wgrad(c, gemm_tn(gD, gH, gW, dsbuf + (int64_t)b * Ng * Np, Np, Np, g + (int64_t)b * Ng * ldg, ldg, k, dF + (int64_t)b * Np * k));
        if (pad()) {
            launch(c, "unpad_rows_kernel", 0, 8.0 * B * Nf * k, [&]() { return p3d_unpad_rows(dfpad, df, B, Nf, Np, k, c.s); });
            launch(c, "unpad_rows_kernel", 0, 8.0 * B * Nf * ch, [&]() { return p3d_unpad_rows(dhpad, dh, B, Nf, Np, ch, c.s); });
        }
    }
};

}  // namespace

namespace {
void ensure_zero_page() {
    // one page per process; igemm2 reads it for padded rows and channel tails
    if (g_zero_page) return;
    float* p = nullptr;
    HIPCHECK(hipMalloc((void**)&p, 1024));
    HIPCHECK(fill_now(p, 0, 1024, nullptr));      // process-wide, once, before any launch reads it
    g_zero_page = p;
}
}  // namespace

// ==================================================================================================
struct p3d_handle {
    p3d_config cfg;
    hipStream_t stream = nullptr, comm_stream = nullptr, side_stream = nullptr;
    bool side_pooled = true;                  // false: created with a CU mask (tuning builds), destroyed with the handle
    std::vector<hipEvent_t> fork_events;
    hipEvent_t ev_side_done = nullptr, ev_side_bucket = nullptr;
    // Events that only order this handle's own streams on one device: no system-scope fence when they complete (the default
    // writes the caches back for the host and for other devices -- tens of microseconds on the main stream at every hand-over
    // to the side stream; the events that gate the all-reduce and the host keep the default).
    static unsigned local_event_flags() {
        static const bool sysfence = [] { const char* e = p3d_tune_env("P3D_TUNE_EVENT_SYSFENCE"); return e && atoi(e); }();
        return hipEventDisableTiming | (sysfence ? 0u : (unsigned)hipEventDisableSystemFence);
    }
    hipEvent_t new_fork_event() {
        hipEvent_t e = nullptr;
        HIPCHECK(hipEventCreateWithFlags(&e, local_event_flags()));
        fork_events.push_back(e);
        return e;
    }
    std::vector<void*> allocs;
    Perturb perturb;                          // p3d_debug_perturb: g_perturb points here while the hook is on

    std::deque<Param> params;                 // stable addresses
    std::map<std::string, Param*> pindex;
    std::vector<Param*> porder;               // creation order (trainables and states interleaved)
    int64_t n_train = 0, n_state = 0;         // floats in the flat buffers
    float *flat_p = nullptr, *flat_g = nullptr, *flat_m = nullptr, *flat_v = nullptr, *flat_state = nullptr;

    std::deque<Act> acts;
    std::map<std::string, Act*> named;
    std::deque<BN> bns;
    std::deque<GN> gns;
    std::deque<CbamSite> cbams;
    std::deque<char> flags;
    std::map<std::string, int> uniq;

    double* stats_arena = nullptr; int64_t stats_count = 0;
    double* red_arena = nullptr;   int64_t red_count = 0;
    float* bnbuf = nullptr;        int64_t bnbuf_count = 0;      // scale/shift/mean/invstd for every BN
    std::vector<std::function<void()>> late_bind;                // pointer fix-ups after arenas are allocated

    std::vector<Op> ops;
    char *zf = nullptr, *zb = nullptr;          // zero arenas: split-K outputs (forward) / gradients (backward)
    size_t zf_bytes = 0, zb_bytes = 0;
    Act* x_in = nullptr;
    Act* pred = nullptr;
    Act* logits = nullptr;
    float* d_y = nullptr;          // target
    float* d_dlogits = nullptr;
    double* d_loss = nullptr;
    int loss_kind = P3D_LOSS_SMOOTH_L1;      // p3d_set_loss
    float kld_weight = 1.f, cc_weight = 1.f;  // p3d_set_loss_weights (P3D_LOSS_KLD_CC)
    double* d_map_scratch = nullptr;          // P3D_LOSS_KLD_CC: per-map statistics and block partials, planned in head()
    unsigned* d_map_cnt = nullptr;            //   and its arrival counters (zero between launches)
    // P3D_LOSS_SALIENCY: p3d_set_saliency_weights, its scratch (allocated when the kind is first selected) and the fixation
    // bytes [B,T,H,W] of p3d_upload_fixations (allocated by the first upload); nothing of it exists for users of other kinds
    float sal_kld = 1.f, sal_cc = 1.f, sal_nss = 1.f, sal_sim = 0.f;
    double* d_sal_scratch = nullptr;
    unsigned* d_sal_cnt = nullptr;
    unsigned char* d_fix = nullptr;
    bool fix_fresh = false;                   // uploaded since the last p3d_train_step / p3d_backward
    int last_loss_kind = -1;                  // the kind of the last step's or backward's loss launches (p3d_last_loss_terms)
    float lr = 1e-4f, b1 = 0.9f, b2 = 0.999f, eps = 1e-8f;
    int64_t step = 0;                         // completed optimiser steps (every kind)
    int opt_kind = P3D_OPT_ADAM;              // p3d_set_optimizer: Momentum keeps its accumulator in flat_m
    float momentum = 0.9f; int use_nesterov = 0;

    ncclComm_t comm = nullptr;
    hipEvent_t ev_bucket = nullptr, ev_comm_done = nullptr;
    int64_t bucket_floats = 8 << 20;          // 32 MB buckets

    // ---------------------------------------------------------------------------------------------
    template <typename T>
    T* dalloc(int64_t n) {
        void* p = nullptr;
        if (n <= 0) n = 1;
        HIPCHECK(hipMalloc(&p, (size_t)n * sizeof(T)));
        allocs.push_back(p);
        return (T*)p;
    }

    std::string unique(const std::string& base) {
        int k = uniq[base]++;
        return k == 0 ? base : base + "_" + std::to_string(k);
    }

    // BASELINE configs[4] option: 1x1x1 convolutions (forward and input gradient) round their operand fragments to
    // fp16 in registers and run on the fp16 MFMA with fp32 accumulation; storage, weights, statistics, every other
    // conv and all weight gradients stay fp32.  Off by default: the 1e-3 parity target is for the fp32 path.
    bool pointwise_f16 = false;
    std::string var_prefix;      // enclosing tf.variable_scope ("P3D/" for gn/p3d_gn.py:490), part of every variable name
    Param* add_param(const std::string& bare_name, std::vector<int64_t> shape, bool trainable, int init) {
        const std::string name = var_prefix + bare_name;
        if (pindex.count(name)) throw P3dError("duplicate variable " + name);
        params.emplace_back();
        Param* p = &params.back();
        p->name = name; p->shape = shape; p->trainable = trainable; p->init = init;
        p->count = 1;
        for (auto d : shape) p->count *= d;
        int64_t& total = trainable ? n_train : n_state;
        p->off = total;
        total += (p->count + 63) / 64 * 64;          // 256-byte aligned slots
        pindex[name] = p;
        porder.push_back(p);
        return p;
    }

    Act* new_act(const std::string& name, int N, int D, int H, int W, int C, bool with_grad = true) {
        acts.emplace_back();
        Act* a = &acts.back();
        a->name = name; a->N = N; a->D = D; a->H = H; a->W = W; a->C = C; a->ld = C;
        a->p = dalloc<float>(a->rows() * C);
        if (with_grad) a->g = dalloc<float>(a->rows() * C);
        if (!name.empty()) named[name] = a;
        return a;
    }
    Act* new_view(Act* parent, int coff, int C, const std::string& name) {
        acts.emplace_back();
        Act* a = &acts.back();
        *a = *parent;
        a->name = name; a->C = C; a->parent = parent; a->views.clear(); a->last_flag = nullptr;
        a->p = parent->p + coff;
        a->g = parent->g ? parent->g + coff : nullptr;
        parent->views.push_back(a);
        if (!name.empty()) named[name] = a;
        return a;
    }

    // Register a consumer of `a` whose backward adds into a->g.  Returns the flag the consumer reads
    // at backward time: 0 = first writer (overwrite), 1 = accumulate.  Backward runs consumers in
    // reverse registration order, so the newest registration is the writer.
    char* consume(Act* a) {
        flags.push_back(0);
        char* f = &flags.back();
        std::vector<Act*> region{a};
        // A concat buffer's whole-buffer consumer must be its newest one: its input gradient is then the
        // first write of every slice in backward order, and the slices' own consumers add to it.
        if (a->parent && a->parent->whole_consumed)
            throw P3dError("consumer of slice " + a->name + " registered after the consumer of its concat buffer " + a->parent->name);
        if (!a->views.empty()) a->whole_consumed = true;
        if (a->parent) region.push_back(a->parent);
        for (Act* v : a->views) region.push_back(v);
        for (Act* r : region) {
            if (r->last_flag) *r->last_flag = 1;
            r->last_flag = f;
        }
        return f;
    }

    // scratch of the per-sample BatchNorm inference path: two (sum, sumsq) tables and two scale/shift/mean/invstd
    // tables of [batch][widest BN]; ops run one after another on one stream, so they can share it
    double* ps_sums = nullptr; float* ps_tab = nullptr; int64_t ps_nc = 0;
    void ensure_per_sample_scratch() {
        if (ps_sums) return;
        int cmax = 4;
        for (auto& bn : bns) cmax = std::max(cmax, bn.C);
        ps_nc = (int64_t)cfg.batch * cmax;
        ps_sums = dalloc<double>(2 * 2 * ps_nc);
        ps_tab = dalloc<float>(2 * 4 * ps_nc);
    }
    BN* add_bn(const std::string& name_or_empty, int C, bool follows_flag) {
        bns.emplace_back();
        BN* bn = &bns.back();
        bn->name = name_or_empty.empty() ? unique("batch_normalization") : name_or_empty;
        bn->C = C; bn->follows_flag = follows_flag;
        bn->gamma = add_param(bn->name + "/gamma", {C}, true, INIT_ONES);
        bn->beta = add_param(bn->name + "/beta", {C}, true, INIT_ZEROS);
        bn->mm = add_param(bn->name + "/moving_mean", {C}, false, INIT_ZEROS);
        bn->mv = add_param(bn->name + "/moving_variance", {C}, false, INIT_ONES);
        const int64_t o = bnbuf_count; bnbuf_count += 4 * (int64_t)C;
        late_bind.push_back([this, bn, o, C]() {
            bn->scale = bnbuf + o; bn->shift = bnbuf + o + C; bn->mean = bnbuf + o + 2 * C; bn->invstd = bnbuf + o + 3 * C;
        });
        return bn;
    }
    // Reserve room for the producer's per-tile statistics partials of a `rows`-row output (bn_part_cap).
    float* statpart_arena = nullptr; int64_t statpart_count = 0;
    void reserve_stat_parts(BN* bn, int64_t rows) {
        if (bn->part_off >= 0) return;
        bn->part_cap = bn_part_cap(rows, bn->C);
        bn->part_off = statpart_count;
        statpart_count += (int64_t)bn->part_cap * bn->C * 2;
    }
    StatSink bn_sink(BN* bn) {
        if (bn->part_off < 0) throw P3dError("BatchNorm " + bn->name + " has no statistics arena slot");
        StatSink s; s.part = statpart_arena + bn->part_off; s.cap = bn->part_cap; s.nparts = &bn->nparts;
        return s;
    }
    // Producers of tensors that the one-launch small-tensor BN will consume need no statistics epilogue.
    static bool bn_is_small(int64_t rows, int C, bool dropout = false) { return bn_path(rows, C, dropout, 0, 0, 0.f) == BN_SMALL; }
    BN* stats_target(BN* bn, int64_t rows, int C, bool dropout = false) { return bn_is_small(rows, C, dropout) ? nullptr : bn; }
    // The BatchNorm whose slot a producer's epilogue statistics fill, as that launch's sink (held in `sink`); null: the launch writes
    // none.  fused: a fused BatchNorm behind the conv always needs the tile partials (the one-launch small-tensor BN does not).
    const StatSink* epilogue_sink(StatSink& sink, BN* bn, int64_t rows, int C, bool dropout, bool fused = false) {
        if (!bn || !(fused || stats_target(bn, rows, C, dropout))) return nullptr;
        sink = bn_sink(bn);
        return &sink;
    }
    BnParams bn_params(BN* bn) {      // (add_bn lays scale, shift, mean, invstd out as one [4][C] table)
        return bn_layout(bn->gamma->p, bn->beta->p, bn->mm->p, bn->mv->p, bn->scale,
                         bn->part_off >= 0 ? statpart_arena + bn->part_off : nullptr, bn->nparts, bn->C);
    }

    // ---- deferred, grouped weight gradients -------------------------------------------------------
    // A conv's filter gradient needs only its input and its output gradient, both of which stay untouched until the
    // step ends, and nothing waits for it before the all-reduce / optimiser.  So backward does not launch it on the
    // spot: problems queue up and go to the side stream several at a time (p3d_launch_wgrad2_group) -- the four
    // filter gradients of a stage-3 bottleneck offer 320 output tiles together, enough for the 256 CUs without
    // cutting the 784-position reduction.  Flushed when a group is full, before a gradient bucket is handed to the
    // all-reduce, and at the end of backward.
    struct PendingWgrad { WgradArgs a; std::string op; double flops, bytes; };
    std::vector<PendingWgrad> wq;
    std::vector<hipEvent_t> wq_events;          // one fork event per flush of a backward pass, reused every step
    int defer_release_op = -1;                  // backward: side-stream jobs of ops after this one wait until the walk reaches it
    double defer_budget = 0, parked_flops = 0;  // ... up to this many filter-gradient FLOPs (what the encoder's idle CUs can absorb)
    size_t wq_flushes = 0;
    static int64_t wgrad_tiles64(const WgradArgs& a) { return (int64_t)a.ntaps * ((a.K + 63) / 64) * ((a.Nc + 63) / 64); }
    void queue_wgrad(const Ctx& c, const WgradArgs& a0) {
        if (c.dry) return;
        WgradArgs a = a0;
        a.zeros = g_zero_page;
        PendingWgrad pw;
        pw.a = a; pw.op = c.prof ? c.prof->cur_op : std::string();
        wgrad_work(a, pw.flops, pw.bytes);
        static const bool no_group = p3d_tune_env("P3D_NO_WGRAD_GROUP") != nullptr;
        static const int64_t flush_tiles = p3d_tune_env("P3D_WGRAD_FLUSH_TILES") ? atol(p3d_tune_env("P3D_WGRAD_FLUSH_TILES")) : 512;   // tuning: 256 -> 17.25 ms / step, 512 -> 17.0, 1024 with groups of 12 -> 17.1
        const bool alone = no_group || wgrad_tiles64(a) >= 256;      // fills the chip by itself (and may take 128x128 tiles)
        if (alone) flush_wgrads(c);
        wq.push_back(pw);
        int64_t tiles = 0;
        for (auto& q : wq) tiles += wgrad_tiles64(q.a);
        static const int group_max = p3d_tune_env("P3D_WGRAD_GROUP_MAX") ? std::max(1, std::min(P3D_WGRAD_GROUP, atoi(p3d_tune_env("P3D_WGRAD_GROUP_MAX")))) : P3D_WGRAD_GROUP;
        if (alone || (int)wq.size() >= group_max || tiles >= flush_tiles) flush_wgrads(c);
    }
    void flush_wgrads(const Ctx& c) {
        if (wq.empty() || c.dry) { wq.clear(); return; }
        if (wq_flushes >= wq_events.size()) {
            hipEvent_t e = nullptr;
            HIPCHECK(hipEventCreateWithFlags(&e, local_event_flags()));
            wq_events.push_back(e);
        }
        hipEvent_t ev = wq_events[wq_flushes++];
        std::vector<WgradArgs> probs;
        double fl = 0, by = 0;
        for (auto& q : wq) { probs.push_back(q.a); fl += q.flops; by += q.bytes; }
        const char* name = wgrad_group_name(probs);
        if (c.defer) {            // parked: it will run beside the encoder's chain of small launches -- low residency (conv_wgrad2.hip)
            for (auto& pr : probs) pr.polite = 1;
            parked_flops += fl;
        }
        on_side_stream(c, ev, [=](const Ctx& sc) {          // by value: the job may be parked (Ctx::defer)
            launch_wgrad_group(sc, probs, name, fl, by);
        });
        wq.clear();
    }

    // ---- BatchNorm fused into the bottleneck convs' operand paths (p3d_kernels.h, conv_igemm2.hip) ---------------
    // The bn -> relu pairs INSIDE a bottleneck (p3d.py:56-81,88-97: after conv1, convS, convT) are not passes of their own
    // when fuse_bn is on: the consumer conv normalises its A fragments on the fly, the input-gradient launches gate and
    // reduce, the next input-gradient / filter-gradient launch applies BatchNorm's backward on its operand path.  The
    // unfused ops stay in the graph (per-sample inference statistics, p3d_set_bn_fusion(h, 0), parity tests of one
    // path against the other) and run instead when Ctx::fuse is off.
    // OFF by default: measured on MI355X at 8 clips of 16x112x112 (profiles/r03_bn_fusion_ab.json) the fused forward is a wash
    // (17.42-17.52 vs 17.33-17.36 ms / step, 96 launches fewer) and the fully fused step is slower (18.4-18.5 ms, 192 fewer):
    // with one wave per SIMD nothing hides the operand work, so it costs about what the removed launches did.
    bool fuse_bn = false;
    bool fuse_bn_bwd = false;         // p3d_set_bn_fusion(h, 2): the backward pass fused too
    bool last_forward_fused = false;
    bool pred_ready = false;          // a forward pass has been issued: `pred` holds a prediction (p3d_pred_maps_u8 refuses before)
    // Only bottlenecks whose inner tensors have at most this many rows are built fusable: there a BatchNorm pass is a
    // latency-bound launch of its own (stage 3 at 8 clips of 16x112x112: 784 rows), while on big tensors the passes stream at
    // HBM speed and the convs are throughput-bound, so per-step operand work costs more than the passes it removes
    // (measured per stage).  P3D_FUSE_MAX_ROWS (read once, at p3d_create) overrides it for A/B runs.
    int64_t fuse_max_rows = 2048;
    struct FuseSrc { Act* y = nullptr; BN* bn = nullptr; int pub = 0; };   // pub: 0 read the published scale / shift, 1 fold the partials and publish, 2 fold only
    struct ConvFuse {
        int at = 0;                          // P3D_AT_RELU1 / P3D_AT_RELU2 on the conv's input
        FuseSrc src[2];
        int ngate = 0; FuseSrc gate[2];      // input-gradient epilogue: gated result -> gate.y->g, partial sums -> gate.bn
        Act* raw = nullptr; char* raw_flag = nullptr;     // ... and the raw result there (added to it when *raw_flag)
        bool accum_in = false;               // the raw gradient another consumer left in x->g is added before gating
        BN* out_bn = nullptr;                // the conv's output feeds a fused BatchNorm: dy = k1*g + k2*y + k3 on the operand paths
        bool any() const { return at != 0 || out_bn != nullptr; }
    };
    void make_fusable(BN* bn, int64_t rows) {
        if (bn->fusable) return;
        bn->fusable = true;
        reserve_stat_parts(bn, rows);
        bn->gpart_cap = (int)(rows / 64 + 8);
        bn->gpart_off = statpart_count;
        statpart_count += (int64_t)bn->gpart_cap * bn->C * 2;
        const int64_t o = bnbuf_count; bnbuf_count += 3 * (int64_t)bn->C;
        late_bind.push_back([this, bn, o]() { bn->coef = bnbuf + o; });
    }
    // forward: many partials -> one finalize launch that every consumer then reads (must precede a fork to the side stream)
    std::map<BN*, bool> fwd_finalized, grad_finalized;      // per pass: the published values are complete
    // the plain descriptors of the launch builders above (fused_bn_fold, fused_bn_grad_fold, ...)
    FusedBn fused_bn_desc(const FuseSrc& s, int64_t rows, const Ctx& c) {
        BN* bn = s.bn;
        FusedBn d;
        d.gamma = bn->gamma->p; d.beta = bn->beta->p; d.C = bn->C;
        d.scale = bn->scale; d.shift = bn->shift; d.mean = bn->mean; d.invstd = bn->invstd;
        d.moving_mean = bn->mm->p; d.moving_var = bn->mv->p;
        d.part = statpart_arena + bn->part_off; d.nparts = bn->nparts;
        d.rows = rows; d.pub = s.pub; d.update_moving = c.update_moving;
        return d;
    }
    FusedBnGrad fused_grad_desc(BN* bn, int64_t rows) {
        FusedBnGrad d;
        d.gamma = bn->gamma->p; d.mean = bn->mean; d.invstd = bn->invstd; d.C = bn->C;
        d.coef = bn->coef; d.dgamma = bn->gamma->g; d.dbeta = bn->beta->g;
        d.part = statpart_arena + bn->gpart_off; d.nparts = bn->gnparts; d.rows = rows;
        return d;
    }
    void fused_prefinalize(const Ctx& c, const ConvFuse& cf, int64_t rows) {
        if (c.dry) return;
        for (int q = 0; q < (cf.at == P3D_AT_RELU2 ? 2 : 1); ++q) {
            BN* bn = cf.src[q].bn;
            if (cf.src[q].pub != 1) continue;
            bn->used_batch = true;
            fwd_finalized[bn] = fused_bn_prefinalize(c, fused_bn_desc(cf.src[q], rows, c));
        }
    }
    BnGate bn_gate(const FuseSrc& s) {
        BnGate g;
        memset(&g, 0, sizeof(g));
        g.y = s.y->p; g.ldy = s.y->ld;
        g.scale = s.bn->scale; g.shift = s.bn->shift; g.mean = s.bn->mean; g.invstd = s.bn->invstd;
        g.out = s.y->g; g.ldo = s.y->ld;
        g.part = statpart_arena + s.bn->gpart_off;
        return g;
    }

    std::vector<IgemmArgs> sib_pending;      // a sibling pair's first launch, waiting for the second (conv(): sibling)

#include "net_ops.inc"
#include "net_gn.inc"
#include "net_graphs.inc"
#include "net_plan.inc"
#include "net_postcfg.inc"
#include "net_prior.inc"
#include "net_fixpool.inc"
#include "net_video.inc"
#include "net_trainset.inc"
#include "net_sched.inc"
};

#include "net_abi.inc"
#include "net_carve.inc"
#include "net_readout.inc"
#include "net_shots.inc"
