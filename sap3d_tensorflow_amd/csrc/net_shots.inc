// ---- shot boundaries of 8-bit frames (shots.hip; the law in include/p3d_hip.h): one check and one launch description for
// p3d_shot_distances_u8, p3d_shot_cuts and the hooks --------------------------------------------------------------------------------
namespace {
void shots_shape_check(const char* who, int n, int H, int W, int gy, int gx) {
    if (n < 1 || n > 65535) throw P3dError(std::string(who) + ": 1 .. 65535 frames");
    if (H < 1 || W < 1) throw P3dError(std::string(who) + ": empty frame");
    if ((long long)H * W > P3D_SHOTS_MAX_PIXELS) throw P3dError(std::string(who) + ": H * W exceeds 2^28, the bound that keeps a distance in 32 bits");
    if (gy < 1 || gy > std::min(P3D_SHOTS_MAX_GRID, H) || gx < 1 || gx > std::min(P3D_SHOTS_MAX_GRID, W))
        throw P3dError(std::string(who) + ": the grid is " + std::to_string(gy) + " x " + std::to_string(gx) + "; 1 <= grid_y <= min(4, H) and 1 <= grid_x <= min(4, W)");
}
// the four numbers of the decision (the grid is checked against a frame's shape where there is one)
void shots_rule_check(const char* who, const int* cfg) {
    if (cfg[P3D_SHOTS_THRESHOLD] < 1 || cfg[P3D_SHOTS_THRESHOLD] > 1000) throw P3dError(std::string(who) + ": the threshold is 1 .. 1000 permille of 6 H W");
    if (cfg[P3D_SHOTS_WINDOW] < 0 || cfg[P3D_SHOTS_WINDOW] > 32) throw P3dError(std::string(who) + ": the window is 0 .. 32 frames");
    if (cfg[P3D_SHOTS_RATIO] < 256 || cfg[P3D_SHOTS_RATIO] > 65535) throw P3dError(std::string(who) + ": the ratio is 256 .. 65535 (q8)");
    if (cfg[P3D_SHOTS_MIN_LENGTH] < 1) throw P3dError(std::string(who) + ": the minimum length is at least 1 frame");
}
// a shot table over F frames: starts[0] == 0, strictly ascending, every start below F
void shots_table_check(const char* who, const int32_t* starts, int n_shots, int F) {
    if (n_shots < 1 || n_shots > F) throw P3dError(std::string(who) + ": 1 .. F shots");
    if (!starts) throw P3dError("null argument");
    if (starts[0] != 0) throw P3dError(std::string(who) + ": the first shot starts at frame 0, not at " + std::to_string(starts[0]));
    for (int k = 1; k < n_shots; ++k) {
        if (starts[k] <= starts[k - 1]) throw P3dError(std::string(who) + ": shot starts ascend strictly; start " + std::to_string(k) + " does not");
        if (starts[k] >= F) throw P3dError(std::string(who) + ": shot start " + std::to_string(starts[k]) + " is outside [0, " + std::to_string(F) + ")");
    }
}
ShotsArgs shots_args(int n, int H, int W, int gy, int gx, int ballot) {
    ShotsArgs a;
    a.n = n; a.H = H; a.W = W; a.gy = gy; a.gx = gx; a.ballot = ballot;
    const ShotsPlan p = p3d_shots_plan(H, W, gy, gx, n);
    a.rows_per_block = p.rows_per_block; a.blocks_per_frame = p.blocks_per_frame; a.frames_per_chunk = p.frames_per_chunk;
    return a;
}
size_t shots_tab_words(const ShotsArgs& a) { return (size_t)(p3d_shots_plan(a.H, a.W, a.gy, a.gx, a.n).scratch_bytes / 4); }
ShotCutArgs shot_cut_args(const int* cfg, int F, long long P, int cap) {
    ShotCutArgs c;
    c.F = F; c.P = P; c.cap = cap;
    c.threshold_permille = cfg[P3D_SHOTS_THRESHOLD]; c.window = cfg[P3D_SHOTS_WINDOW]; c.ratio_q8 = cfg[P3D_SHOTS_RATIO];
    c.min_length = cfg[P3D_SHOTS_MIN_LENGTH];
    return c;
}
// ---- gradual transitions: the same three for p3d_shot_signals_u8, p3d_shot_transitions, p3d_video_detect_transitions and the hooks
void shots_lag_check(const char* who, int lag) {
    if (lag != 0 && (lag < 2 || lag > P3D_SHOTS_MAX_LAG)) throw P3dError(std::string(who) + ": the lag is 0 (dissolves off) or 2 .. 64 frames");
}
void gradual_rule_check(const char* who, const int* g) {
    shots_lag_check(who, g[P3D_GRADUAL_LAG]);
    if (g[P3D_GRADUAL_HIGH] < 1 || g[P3D_GRADUAL_HIGH] > 1000) throw P3dError(std::string(who) + ": high is 1 .. 1000 permille of 6 H W");
    if (g[P3D_GRADUAL_DIP] < 1 || g[P3D_GRADUAL_DIP] > 256) throw P3dError(std::string(who) + ": dip is 1 .. 256 (q8)");
    if (g[P3D_GRADUAL_MONO] < 0 || g[P3D_GRADUAL_MONO] > 65535) throw P3dError(std::string(who) + ": mono is 0 .. 65535 (q8)");
    if (g[P3D_GRADUAL_MONO_MIN] < 0) throw P3dError(std::string(who) + ": mono_min is 0 (fades off) or a number of frames");
}
ShotSignalsArgs shot_signals_args(int n, int H, int W, int gy, int gx, int lag) {
    ShotSignalsArgs a;
    a.cut = shots_args(n, H, W, gy, gx, P3D_SHOTS_BALLOT);
    a.lag = lag;
    return a;
}
size_t shot_signals_tab_words(const ShotSignalsArgs& a) { return (size_t)(p3d_transitions_plan(a.cut.gy, a.cut.gx, a.cut.n, a.lag).scratch_bytes / 4); }
ShotTransitionArgs shot_transition_args(const int* cfg, const int* g, int F, long long P, int cap) {
    ShotTransitionArgs t;
    t.cut = shot_cut_args(cfg, F, P, cap);
    t.lag = g[P3D_GRADUAL_LAG]; t.high_permille = g[P3D_GRADUAL_HIGH]; t.dip_q8 = g[P3D_GRADUAL_DIP]; t.mono_q8 = g[P3D_GRADUAL_MONO];
    t.mono_min = g[P3D_GRADUAL_MONO_MIN];
    return t;
}
}  // namespace
extern "C" {

int p3d_shot_distances_u8(int device, const unsigned char* frames, int n, int H, int W, int grid_y, int grid_x, uint32_t* D) {
    API_BEGIN
    const char* who = "shot_distances_u8";
    if (!frames || !D) throw P3dError("null argument");
    shots_shape_check(who, n, H, W, grid_y, grid_x);
    metric_args(device, frames, frames, 1, 1, D);
    ShotsArgs a = shots_args(n, H, W, grid_y, grid_x, P3D_SHOTS_BALLOT);
    DevArr<unsigned char> df((size_t)n * H * W * 3, frames);
    DevArr<uint32_t> dD((size_t)n);
    DevArr<unsigned> tabs(shots_tab_words(a));
    a.frames = df.p; a.D = dD.p; a.tabs = tabs.p;
    HIPCHECK(p3d_shots_launch(a, nullptr));
    dD.get(D, (size_t)n);
    API_END
}

int p3d_debug_shot_distances_u8(int device, const unsigned char* frames, int n, int H, int W, int grid_y, int grid_x, int offset, int ballot,
                                uint32_t* D) {
    API_BEGIN
    const char* who = "debug_shot_distances_u8";
    if (!frames || !D) throw P3dError("null argument");
    shots_shape_check(who, n, H, W, grid_y, grid_x);
    offset_check(who, offset);
    if (ballot != 0 && ballot != 1) throw P3dError(std::string(who) + ": ballot is 0 or 1");
    metric_args(device, frames, frames, 1, 1, D);
    ShotsArgs a = shots_args(n, H, W, grid_y, grid_x, ballot);
    Guarded<unsigned char> df((size_t)n * H * W * 3, 16, (size_t)offset, frames);
    Guarded<uint32_t> dD((size_t)n, 16, 0, nullptr);
    Guarded<unsigned> tabs(shots_tab_words(a), 16, 0, nullptr);
    a.frames = df.data(); a.D = dD.data(); a.tabs = tabs.data();
    HIPCHECK(p3d_shots_launch(a, nullptr));
    dD.back(D, who);
    tabs.back(nullptr, who);
    df.unchanged(who);
    API_END
}

int p3d_debug_shots_plan(int H, int W, int grid_y, int grid_x, int n, int* rows_per_block, int* blocks_per_frame, int* frames_per_chunk,
                         int64_t* scratch_bytes) {
    API_BEGIN
    if (!rows_per_block || !blocks_per_frame || !frames_per_chunk || !scratch_bytes) throw P3dError("null argument");
    shots_shape_check("debug_shots_plan", n, H, W, grid_y, grid_x);
    const ShotsPlan p = p3d_shots_plan(H, W, grid_y, grid_x, n);
    *rows_per_block = p.rows_per_block; *blocks_per_frame = p.blocks_per_frame; *frames_per_chunk = p.frames_per_chunk;
    *scratch_bytes = (int64_t)p.scratch_bytes;
    API_END
}

int p3d_debug_shots_time(int device, const unsigned char* frames, int n, int H, int W, int grid_y, int grid_x, int reps, double* signal_ms,
                         double* ballot_ms, double* copy_ms) {
    API_BEGIN
    const char* who = "debug_shots_time";
    if (!frames || !signal_ms || !ballot_ms || !copy_ms) throw P3dError("null argument");
    shots_shape_check(who, n, H, W, grid_y, grid_x);
    if (reps < 1 || reps > 1000) throw P3dError(std::string(who) + ": 1 .. 1000 repetitions");
    metric_args(device, frames, frames, 1, 1, signal_ms);
    const size_t bytes = (size_t)n * H * W * 3;
    ShotsArgs a = shots_args(n, H, W, grid_y, grid_x, 0);
    DevArr<unsigned char> df(bytes, frames), dcopy(bytes);
    DevArr<uint32_t> dD((size_t)n);
    DevArr<unsigned> tabs(shots_tab_words(a));
    a.frames = df.p; a.D = dD.p; a.tabs = tabs.p;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIPCHECK(hipEventCreate(&e0));
    HIPCHECK(hipEventCreate(&e1));
    auto timed = [&](const std::function<void()>& work) {
        float ms = 0.f;
        HIPCHECK(hipEventRecord(e0, nullptr));
        work();
        HIPCHECK(hipEventRecord(e1, nullptr));
        HIPCHECK(hipEventSynchronize(e1));
        HIPCHECK(hipEventElapsedTime(&ms, e0, e1));
        return (double)ms;
    };
    // one untimed round warms all three, then they alternate
    for (int r = -1; r < reps; ++r) {
        a.ballot = 0;
        const double t0 = timed([&] { HIPCHECK(p3d_shots_launch(a, nullptr)); });
        a.ballot = 1;
        const double t1 = timed([&] { HIPCHECK(p3d_shots_launch(a, nullptr)); });
        const double t2 = timed([&] { HIPCHECK(hipMemcpyAsync(dcopy.p, df.p, bytes, hipMemcpyDeviceToDevice, nullptr)); });
        if (r >= 0) { signal_ms[r] = t0; ballot_ms[r] = t1; copy_ms[r] = t2; }
    }
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    API_END
}

int p3d_shot_cuts(int device, const uint32_t* D, int F, int64_t P, const int cfg[6], int32_t* starts, int cap, int* n_shots) {
    API_BEGIN
    const char* who = "shot_cuts";
    if (!D || !cfg || !starts || !n_shots) throw P3dError("null argument");
    if (F < 1 || F > 65535) throw P3dError(std::string(who) + ": 1 .. 65535 frames");
    if (P < 1 || P > P3D_SHOTS_MAX_PIXELS) throw P3dError(std::string(who) + ": P = H * W is 1 .. 2^28");
    if (cap < 1) throw P3dError(std::string(who) + ": room for at least one start");
    shots_rule_check(who, cfg);
    metric_args(device, D, cfg, 1, 1, starts);
    ShotCutArgs c = shot_cut_args(cfg, F, (long long)P, cap);
    Guarded<uint32_t> dD((size_t)F, 16, 0, D);
    Guarded<unsigned> cand((size_t)F, 16, 0, nullptr);
    Guarded<int32_t> ds((size_t)cap, 16, 0, nullptr), dn(1, 16, 0, nullptr);
    c.D = dD.data(); c.cand = cand.data(); c.starts = ds.data(); c.n_shots = dn.data();
    HIPCHECK(p3d_shot_cuts_launch(c, nullptr));
    std::vector<int32_t> got((size_t)cap);
    int32_t count = 0;
    ds.back(got.data(), who); dn.back(&count, who); cand.back(nullptr, who); dD.unchanged(who);
    std::copy(got.begin(), got.begin() + std::min(cap, (int)count), starts);
    *n_shots = (int)count;
    API_END
}

int p3d_temporal_filter_shots(int device, int mode, const p3d_video_temporal* cfg, const float* store, const int32_t* count, int F, int64_t hw,
                              const int32_t* starts, int n_shots, int first, int n, int offset, float* out) {
    API_BEGIN
    const char* who = "temporal_filter_shots";
    if (!store || !out) throw P3dError("null argument");
    if (mode != VIDEO_NEWEST && mode != VIDEO_MEAN) throw P3dError(std::string(who) + ": mode " + std::to_string(mode) + " is neither P3D_VIDEO_NEWEST (0) nor P3D_VIDEO_MEAN (1)");
    const p3d_handle::TemporalCfg t = p3d_handle::TemporalCfg::parse(cfg);
    if (!t.on()) throw P3dError(std::string(who) + ": needs a kind (GAUSS or EMA)");
    if (F < 1 || hw < 1 || (int64_t)F * hw > (int64_t)1 << 31) throw P3dError(std::string(who) + ": bad shape");
    shots_table_check(who, starts, n_shots, F);
    std::vector<int32_t> ones;
    if (!count) { ones.assign((size_t)F, 1); count = ones.data(); }
    p3d_handle::TemporalCfg::check_shots(who, t, F, first, n, count, starts, n_shots);
    video_hook_device(device, offset);
    const std::vector<int> runs = p3d_video_temporal_runs(t.set.kind, t.r, hw, F, first, n, starts, n_shots);
    const int64_t ns = (int64_t)F * hw, no = (int64_t)n * hw;
    Guarded<float> sb((size_t)ns, 8, (size_t)offset, store), ob((size_t)no, 8, (size_t)offset, nullptr);
    Guarded<int32_t> cb((size_t)F, 8, 0, count);
    Guarded<int> rb(runs.size(), 8, 0, runs.data());
    const VideoTemporalArgs a = p3d_handle::TemporalCfg::args(t, sb.data(), mode == VIDEO_MEAN ? cb.data() : nullptr, ob.data(), F, hw, first, n);
    HIPCHECK(p3d_video_temporal_shots_launch(a, rb.data(), (int)(runs.size() / 4), nullptr));
    HIPCHECK(hipDeviceSynchronize());
    sb.unchanged(who); cb.unchanged(who); rb.unchanged(who);
    ob.back(out, who);
    API_END
}

// ---- gradual transitions at op level --------------------------------------------------------------------------------------------------
int p3d_shot_signals_u8(int device, const unsigned char* frames, int n, int H, int W, int grid_y, int grid_x, int lag, uint32_t* D, uint32_t* E,
                        int64_t* v) {
    API_BEGIN
    const char* who = "shot_signals_u8";
    if (!frames || !D || !E || !v) throw P3dError("null argument");
    shots_shape_check(who, n, H, W, grid_y, grid_x);
    shots_lag_check(who, lag);
    metric_args(device, frames, frames, 1, 1, D);
    ShotSignalsArgs a = shot_signals_args(n, H, W, grid_y, grid_x, lag);
    DevArr<unsigned char> df((size_t)n * H * W * 3, frames);
    DevArr<uint32_t> dD((size_t)n), dE((size_t)n);
    DevArr<long long> dv((size_t)n);
    DevArr<unsigned> tabs(shot_signals_tab_words(a));
    a.cut.frames = df.p; a.cut.D = dD.p; a.E = dE.p; a.v = dv.p; a.cut.tabs = tabs.p;
    HIPCHECK(p3d_shot_signals_launch(a, nullptr));
    dD.get(D, (size_t)n); dE.get(E, (size_t)n); dv.get(reinterpret_cast<long long*>(v), (size_t)n);
    API_END
}

int p3d_debug_shot_signals_u8(int device, const unsigned char* frames, int n, int H, int W, int grid_y, int grid_x, int lag, int offset,
                              uint32_t* D, uint32_t* E, int64_t* v) {
    API_BEGIN
    const char* who = "debug_shot_signals_u8";
    if (!frames || !D || !E || !v) throw P3dError("null argument");
    shots_shape_check(who, n, H, W, grid_y, grid_x);
    shots_lag_check(who, lag);
    offset_check(who, offset);
    metric_args(device, frames, frames, 1, 1, D);
    ShotSignalsArgs a = shot_signals_args(n, H, W, grid_y, grid_x, lag);
    Guarded<unsigned char> df((size_t)n * H * W * 3, 16, (size_t)offset, frames);
    Guarded<uint32_t> dD((size_t)n, 16, 0, nullptr), dE((size_t)n, 16, 0, nullptr);
    Guarded<long long> dv((size_t)n, 16, 0, nullptr);
    Guarded<unsigned> tabs(shot_signals_tab_words(a), 16, 0, nullptr);
    a.cut.frames = df.data(); a.cut.D = dD.data(); a.E = dE.data(); a.v = dv.data(); a.cut.tabs = tabs.data();
    HIPCHECK(p3d_shot_signals_launch(a, nullptr));
    dD.back(D, who); dE.back(E, who); dv.back(reinterpret_cast<long long*>(v), who);
    tabs.back(nullptr, who);
    df.unchanged(who);
    API_END
}

int p3d_debug_transitions_plan(int H, int W, int grid_y, int grid_x, int n, int lag, int* tables, int64_t* scratch_bytes) {
    API_BEGIN
    if (!tables || !scratch_bytes) throw P3dError("null argument");
    shots_shape_check("debug_transitions_plan", n, H, W, grid_y, grid_x);
    shots_lag_check("debug_transitions_plan", lag);
    const TransitionsPlan p = p3d_transitions_plan(grid_y, grid_x, n, lag);
    *tables = p.tables;
    *scratch_bytes = (int64_t)p.scratch_bytes;
    API_END
}

int p3d_debug_transitions_time(int device, const unsigned char* frames, int n, int H, int W, int grid_y, int grid_x, int lag, int reps,
                               double* cut_ms, double* signal_ms) {
    API_BEGIN
    const char* who = "debug_transitions_time";
    if (!frames || !cut_ms || !signal_ms) throw P3dError("null argument");
    shots_shape_check(who, n, H, W, grid_y, grid_x);
    shots_lag_check(who, lag);
    if (reps < 1 || reps > 1000) throw P3dError(std::string(who) + ": 1 .. 1000 repetitions");
    metric_args(device, frames, frames, 1, 1, cut_ms);
    ShotSignalsArgs a = shot_signals_args(n, H, W, grid_y, grid_x, lag);
    ShotsArgs c = a.cut;
    DevArr<unsigned char> df((size_t)n * H * W * 3, frames);
    DevArr<uint32_t> dD((size_t)n), dE((size_t)n);
    DevArr<long long> dv((size_t)n);
    DevArr<unsigned> tabs(shot_signals_tab_words(a));      // at least the cut signal's tables
    a.cut.frames = c.frames = df.p; a.cut.D = c.D = dD.p; a.cut.tabs = c.tabs = tabs.p; a.E = dE.p; a.v = dv.p;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIPCHECK(hipEventCreate(&e0));
    HIPCHECK(hipEventCreate(&e1));
    auto timed = [&](const std::function<void()>& work) {
        float ms = 0.f;
        HIPCHECK(hipEventRecord(e0, nullptr));
        work();
        HIPCHECK(hipEventRecord(e1, nullptr));
        HIPCHECK(hipEventSynchronize(e1));
        HIPCHECK(hipEventElapsedTime(&ms, e0, e1));
        return (double)ms;
    };
    for (int r = -1; r < reps; ++r) {                       // one untimed round warms both, then they alternate
        const double t0 = timed([&] { HIPCHECK(p3d_shots_launch(c, nullptr)); });
        const double t1 = timed([&] { HIPCHECK(p3d_shot_signals_launch(a, nullptr)); });
        if (r >= 0) { cut_ms[r] = t0; signal_ms[r] = t1; }
    }
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    API_END
}

int p3d_shot_transitions(int device, const uint32_t* D, const uint32_t* E, const int64_t* v, int F, int64_t P, const int cfg[6], const int gcfg[5],
                         int32_t* starts, int32_t* kinds, int cap, int* n_shots) {
    API_BEGIN
    const char* who = "shot_transitions";
    if (!D || !E || !v || !cfg || !gcfg || !starts || !kinds || !n_shots) throw P3dError("null argument");
    if (F < 1 || F > 65535) throw P3dError(std::string(who) + ": 1 .. 65535 frames");
    if (P < 1 || P > P3D_SHOTS_MAX_PIXELS) throw P3dError(std::string(who) + ": P = H * W is 1 .. 2^28");
    if (cap < 1) throw P3dError(std::string(who) + ": room for at least one start");
    shots_rule_check(who, cfg);
    gradual_rule_check(who, gcfg);
    for (int f = 0; f < F; ++f)
        if (v[f] < 0 || v[f] >= (int64_t)1 << 40) throw P3dError(std::string(who) + ": v[" + std::to_string(f) + "] is outside [0, 2^40)");
    metric_args(device, D, cfg, 1, 1, starts);
    ShotTransitionArgs t = shot_transition_args(cfg, gcfg, F, (long long)P, cap);
    Guarded<uint32_t> dD((size_t)F, 16, 0, D), dE((size_t)F, 16, 0, E);
    Guarded<long long> dv((size_t)F, 16, 0, reinterpret_cast<const long long*>(v));
    Guarded<unsigned> flags((size_t)F, 16, 0, nullptr), marks((size_t)F, 16, 0, nullptr);
    Guarded<int32_t> ds((size_t)cap, 16, 0, nullptr), dk((size_t)cap, 16, 0, nullptr), dn(1, 16, 0, nullptr);
    t.cut.D = dD.data(); t.E = dE.data(); t.v = dv.data(); t.cut.cand = flags.data(); t.marks = marks.data();
    t.cut.starts = ds.data(); t.kinds = dk.data(); t.cut.n_shots = dn.data();
    HIPCHECK(p3d_shot_transitions_launch(t, nullptr));
    std::vector<int32_t> got((size_t)cap), gotk((size_t)cap);
    int32_t count = 0;
    ds.back(got.data(), who); dk.back(gotk.data(), who); dn.back(&count, who); flags.back(nullptr, who); marks.back(nullptr, who);
    dD.unchanged(who); dE.unchanged(who); dv.unchanged(who);
    std::copy(got.begin(), got.begin() + std::min(cap, (int)count), starts);
    std::copy(gotk.begin(), gotk.begin() + std::min(cap, (int)count), kinds);
    *n_shots = (int)count;
    API_END
}

// ---- the open video's shot table ----------------------------------------------------------------------------------------------------
int p3d_video_set_shots(p3d_handle* h, const int32_t* starts, int n_shots) {
    API_BEGIN
    const char* who = "video_set_shots";
    if (!h) throw P3dError("null argument");
    h->video.need_open(who);
    if (!starts) { h->video.shots.clear(); h->video.shot_kinds.clear(); return 0; }
    shots_table_check(who, starts, n_shots, h->video.F);
    h->video.shots.assign(starts, starts + n_shots);
    h->video.shot_kinds.clear();
    API_END
}

int p3d_video_get_shots(p3d_handle* h, int32_t* starts, int cap, int* n_shots) {
    API_BEGIN
    const char* who = "video_get_shots";
    if (!h || !n_shots) throw P3dError("null argument");
    h->video.need_open(who);
    if (starts && cap < 0) throw P3dError(std::string(who) + ": a negative cap");
    if (starts) std::copy(h->video.shots.begin(), h->video.shots.begin() + std::min((size_t)cap, h->video.shots.size()), starts);
    *n_shots = (int)h->video.shots.size();
    API_END
}

int p3d_video_detect_shots(p3d_handle* h, const int cfg[6], uint32_t* D_out, int32_t* starts_out, int cap, int* n_shots, int install) {
    API_BEGIN
    const char* who = "video_detect_shots";
    if (!h || !cfg || !n_shots) throw P3dError("null argument");
    h->video.need_open(who);
    need_kept_source(h, who);
    const int F = h->video.F, H = h->video.H0, W = h->video.W0;
    shots_shape_check(who, F, H, W, cfg[P3D_SHOTS_GRID_Y], cfg[P3D_SHOTS_GRID_X]);
    shots_rule_check(who, cfg);
    if (starts_out && cap < 1) throw P3dError(std::string(who) + ": room for at least one start");
    kept_source(h, who, 0, F, H, W, "reads");
    HIPCHECK(hipSetDevice(h->cfg.device));
    const hipStream_t s = h->stream;
    ShotsArgs a = shots_args(F, H, W, cfg[P3D_SHOTS_GRID_Y], cfg[P3D_SHOTS_GRID_X], P3D_SHOTS_BALLOT);
    ShotCutArgs c = shot_cut_args(cfg, F, (long long)H * W, F);
    const size_t words = shots_tab_words(a);
    unsigned* tabs = nullptr;
    carve_scratch(s, 0, [&](Carve& cv) {
        tabs = cv.take<unsigned>(words);
        a.D = cv.take<uint32_t>((size_t)F);
        c.cand = cv.take<unsigned>((size_t)F);
        c.starts = cv.take<int32_t>((size_t)F);
        c.n_shots = cv.take<int32_t>(1);
    });
    a.frames = h->video.source; a.tabs = tabs; c.D = a.D;
    h->shots_timer.ev.create();
    HIPCHECK(hipEventRecord(h->shots_timer.ev[0], s));
    HIPCHECK(p3d_shots_launch(a, s));
    HIPCHECK(hipEventRecord(h->shots_timer.ev[1], s));
    HIPCHECK(p3d_shot_cuts_launch(c, s));
    HIPCHECK(hipEventRecord(h->shots_timer.ev[2], s));
    h->shots_timer.timed = true;
    std::vector<int32_t> starts((size_t)F);
    int32_t count = 0;
    HIPCHECK(copy_now(&count, c.n_shots, sizeof(count), hipMemcpyDeviceToHost, s));
    HIPCHECK(copy_now(starts.data(), c.starts, (size_t)F * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (D_out) HIPCHECK(copy_now(D_out, a.D, (size_t)F * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (count < 1 || count > F) throw P3dError(std::string(who) + ": the decision returned no table");
    starts.resize((size_t)count);
    if (starts_out) std::copy(starts.begin(), starts.begin() + std::min(cap, (int)count), starts_out);
    *n_shots = (int)count;
    if (install) {
        shots_table_check(who, starts.data(), (int)count, F);
        h->video.shots = starts;
        h->video.shot_kinds.clear();
    }
    API_END
}

int p3d_video_detect_transitions(p3d_handle* h, const int cfg[6], const int gcfg[5], uint32_t* D_out, uint32_t* E_out, int64_t* v_out,
                                 int32_t* starts_out, int32_t* kinds_out, int cap, int* n_shots, int install) {
    API_BEGIN
    const char* who = "video_detect_transitions";
    if (!h || !cfg || !gcfg || !n_shots) throw P3dError("null argument");
    h->video.need_open(who);
    need_kept_source(h, who);
    const int F = h->video.F, H = h->video.H0, W = h->video.W0;
    shots_shape_check(who, F, H, W, cfg[P3D_SHOTS_GRID_Y], cfg[P3D_SHOTS_GRID_X]);
    shots_rule_check(who, cfg);
    gradual_rule_check(who, gcfg);
    if ((starts_out || kinds_out) && cap < 1) throw P3dError(std::string(who) + ": room for at least one start");
    kept_source(h, who, 0, F, H, W, "reads");
    HIPCHECK(hipSetDevice(h->cfg.device));
    const hipStream_t s = h->stream;
    ShotSignalsArgs a = shot_signals_args(F, H, W, cfg[P3D_SHOTS_GRID_Y], cfg[P3D_SHOTS_GRID_X], gcfg[P3D_GRADUAL_LAG]);
    ShotTransitionArgs t = shot_transition_args(cfg, gcfg, F, (long long)H * W, F);
    const size_t words = shot_signals_tab_words(a);
    carve_scratch(s, 0, [&](Carve& cv) {
        a.cut.tabs = cv.take<unsigned>(words);
        a.cut.D = cv.take<uint32_t>((size_t)F);
        a.E = cv.take<uint32_t>((size_t)F);
        a.v = cv.take<long long>((size_t)F);
        t.cut.cand = cv.take<unsigned>((size_t)F);
        t.marks = cv.take<unsigned>((size_t)F);
        t.cut.starts = cv.take<int32_t>((size_t)F);
        t.kinds = cv.take<int32_t>((size_t)F);
        t.cut.n_shots = cv.take<int32_t>(1);
    });
    a.cut.frames = h->video.source; t.cut.D = a.cut.D; t.E = a.E; t.v = a.v;
    h->shots_timer.ev.create();
    HIPCHECK(hipEventRecord(h->shots_timer.ev[0], s));
    HIPCHECK(p3d_shot_signals_launch(a, s));
    HIPCHECK(hipEventRecord(h->shots_timer.ev[1], s));
    HIPCHECK(p3d_shot_transitions_launch(t, s));
    HIPCHECK(hipEventRecord(h->shots_timer.ev[2], s));
    h->shots_timer.timed = true;
    std::vector<int32_t> starts((size_t)F), kinds((size_t)F);
    int32_t count = 0;
    HIPCHECK(copy_now(&count, t.cut.n_shots, sizeof(count), hipMemcpyDeviceToHost, s));
    if (count < 1 || count > F) throw P3dError(std::string(who) + ": the decision returned no table");
    HIPCHECK(copy_now(starts.data(), t.cut.starts, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHECK(copy_now(kinds.data(), t.kinds, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (D_out) HIPCHECK(copy_now(D_out, a.cut.D, (size_t)F * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (E_out) HIPCHECK(copy_now(E_out, a.E, (size_t)F * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (v_out) HIPCHECK(copy_now(v_out, a.v, (size_t)F * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    starts.resize((size_t)count); kinds.resize((size_t)count);
    if (starts_out) std::copy(starts.begin(), starts.begin() + std::min(cap, (int)count), starts_out);
    if (kinds_out) std::copy(kinds.begin(), kinds.begin() + std::min(cap, (int)count), kinds_out);
    *n_shots = (int)count;
    if (install) {
        shots_table_check(who, starts.data(), (int)count, F);
        h->video.shots = starts;
        h->video.shot_kinds = kinds;
    }
    API_END
}

int p3d_video_get_shot_kinds(p3d_handle* h, int32_t* kinds, int cap, int* n_shots) {
    API_BEGIN
    const char* who = "video_get_shot_kinds";
    if (!h || !n_shots) throw P3dError("null argument");
    h->video.need_open(who);
    if (kinds && cap < 0) throw P3dError(std::string(who) + ": a negative cap");
    const size_t n = h->video.shots.size();
    for (size_t k = 0; kinds && k < std::min((size_t)cap, n); ++k)
        kinds[k] = !h->video.shot_kinds.empty() ? h->video.shot_kinds[k] : k == 0 ? P3D_SHOT_FIRST : P3D_SHOT_CUT;
    *n_shots = (int)n;
    API_END
}

int p3d_video_shots_last_ms(p3d_handle* h, double* ms) {
    API_BEGIN
    if (!h || !ms) throw P3dError("null argument");
    if (!h->shots_timer.timed) throw P3dError("video_shots_last_ms: no p3d_video_detect_shots has run");
    float t0 = 0.f, t1 = 0.f;
    HIPCHECK(hipEventSynchronize(h->shots_timer.ev[2]));
    HIPCHECK(hipEventElapsedTime(&t0, h->shots_timer.ev[0], h->shots_timer.ev[1]));
    HIPCHECK(hipEventElapsedTime(&t1, h->shots_timer.ev[1], h->shots_timer.ev[2]));
    ms[0] = t0; ms[1] = t1;
    API_END
}

}  // extern "C"
