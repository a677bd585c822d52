// ---- metrics / pre-processing entry points (metrics.hip) -------------------------------------------------------
namespace {
void metric_args(int device, const void* a, const void* b, int n_maps, int n_pix, const void* out) {
    if (!a || !b || !out) throw P3dError("null argument");
    if (n_maps < 1 || n_pix < 1) throw P3dError("metrics need at least one map and one pixel");
    int ndev = 0;
    HIPCHECK(hipGetDeviceCount(&ndev));
    if (ndev <= 0) throw P3dError("no HIP device: libp3dhip has no CPU fallback");
    if (device < 0 || device >= ndev) throw P3dError("bad device ordinal");
    HIPCHECK(hipSetDevice(device));
}
}  // namespace

extern "C" {

int p3d_metric_cc(int device, const float* a, const float* b, int n_maps, int n_pix, double* out) {
    API_BEGIN
    metric_args(device, a, b, n_maps, n_pix, out);
    const size_t n = (size_t)n_maps * n_pix;
    DevArr<float> da(n, a), db(n, b); DevArr<double> dout(n_maps);
    HIPCHECK(p3d_metric_cc(da.p, db.p, n_maps, n_pix, dout.p, nullptr));
    dout.get(out, n_maps);
    API_END
}
int p3d_metric_sim(int device, const float* a, const float* b, int n_maps, int n_pix, double* out) {
    API_BEGIN
    metric_args(device, a, b, n_maps, n_pix, out);
    const size_t n = (size_t)n_maps * n_pix;
    DevArr<float> da(n, a), db(n, b); DevArr<double> dout(n_maps);
    HIPCHECK(p3d_metric_sim(da.p, db.p, n_maps, n_pix, dout.p, nullptr));
    dout.get(out, n_maps);
    API_END
}
int p3d_metric_nss(int device, const float* sal, const float* fix, int n_maps, int n_pix, double* out) {
    API_BEGIN
    metric_args(device, sal, fix, n_maps, n_pix, out);
    const size_t n = (size_t)n_maps * n_pix;
    DevArr<float> da(n, sal), db(n, fix); DevArr<double> dout(n_maps);
    HIPCHECK(p3d_metric_nss(da.p, db.p, n_maps, n_pix, dout.p, nullptr));
    dout.get(out, n_maps);
    API_END
}
int p3d_metric_auc_judd(int device, const float* sal, const float* fix, const float* jitter, int n_maps, int n_pix, double* out) {
    API_BEGIN
    metric_args(device, sal, fix, n_maps, n_pix, out);
    const size_t n = (size_t)n_maps * n_pix;
    const size_t pad = (size_t)p3d_metric_auc_pad(n_pix);
    DevArr<float> da(n, sal), db(n, fix), dj(jitter ? n : 1, jitter), thr(pad * n_maps);
    DevArr<int> cnt((pad + 1) * n_maps);
    DevArr<double> dout(n_maps);
    HIPCHECK(p3d_metric_auc_judd(da.p, db.p, jitter ? dj.p : nullptr, n_maps, n_pix, thr.p, cnt.p, dout.p, nullptr));
    dout.get(out, n_maps);
    API_END
}
int p3d_metric_auc_borji(int device, const float* sal, const float* fix, const int* rand_idx, int n_pix, int n_fix, int n_rep,
                         double step_size, double* out) {
    API_BEGIN
    metric_args(device, sal, fix, 1, n_pix, out);
    if (!rand_idx || n_rep < 1 || !(step_size > 0.0)) throw P3dError("AUC_Borji needs random indices, n_rep >= 1 and a positive step");
    DevArr<float> da(n_pix, sal), db(n_pix, fix);
    DevArr<int> fidx(n_pix), fcount(1);
    HIPCHECK(p3d_metric_fix_index(db.p, n_pix, fidx.p, fcount.p, nullptr));
    int have = 0;
    fcount.get(&have, 1);
    if (have == 0) { for (int i = 0; i < n_rep; ++i) out[i] = NAN; return 0; }      // "no fixation to predict"
    if (have != n_fix) throw P3dError("AUC_Borji: n_fix = " + std::to_string(n_fix) + " but the fixation map has " + std::to_string(have) + " fixated pixels");
    for (size_t i = 0; i < (size_t)n_fix * n_rep; ++i)
        if (rand_idx[i] < 0 || rand_idx[i] >= n_pix) throw P3dError("AUC_Borji: random index out of range");
    DevArr<int> dr((size_t)n_fix * n_rep, rand_idx);
    DevArr<double> dout(n_rep);
    HIPCHECK(p3d_metric_auc_borji(da.p, db.p, dr.p, n_pix, n_fix, n_rep, step_size, fidx.p, dout.p, nullptr));
    dout.get(out, n_rep);
    API_END
}
int p3d_mapf_frames(int device, const unsigned char* bgr, int n, int H0, int W0, const float mean_rgb[3], int H, int W, float* out) {
    API_BEGIN
    metric_args(device, bgr, mean_rgb, 1, 1, out);
    if (n < 1 || H0 < 1 || W0 < 1 || H < 1 || W < 1) throw P3dError("mapf: empty frame");
    DevArr<unsigned char> src((size_t)n * H0 * W0 * 3, bgr);
    DevArr<float> dst((size_t)n * H * W * 3);
    HIPCHECK(p3d_mapf_frames(src.p, n, H0, W0, dst.p, H, W, mean_rgb, nullptr));
    dst.get(out, (size_t)n * H * W * 3);
    API_END
}
int p3d_mapf_density(int device, const unsigned char* grey, int n, int H0, int W0, int H, int W, float* out) {
    API_BEGIN
    metric_args(device, grey, grey, 1, 1, out);
    if (n < 1 || H0 < 1 || W0 < 1 || H < 1 || W < 1) throw P3dError("mapf: empty frame");
    DevArr<unsigned char> src((size_t)n * H0 * W0, grey);
    DevArr<float> dst((size_t)n * H * W);
    HIPCHECK(p3d_mapf_density(src.p, n, H0, W0, dst.p, H, W, nullptr));
    dst.get(out, (size_t)n * H * W);
    API_END
}

// ---- ground-truth resolution (metrics_full.hip) ----------------------------------------------------------------------
}  // extern "C"
namespace {
int next_pow2(int n) { int p = 1; while (p < n) p <<= 1; return p; }
// every scratch buffer of P3dFullMaps / P3dFullBorji; slot offsets and meta come from n_fix[n_maps]
void carve_full(Carve& c, P3dFullMaps& a, P3dFullBorji& r, const std::vector<int>& meta) {
    const int B = a.n_maps;
    size_t slots = 0;
    for (int b = 0; b < B; ++b) slots += next_pow2(meta[b * 3]);
    a.meta = c.take<int>((size_t)B * 3);
    a.partA = c.take<double>((size_t)B * a.nblk * 11);
    a.partB = c.take<double>((size_t)B * a.nblk * 8);
    a.partC = c.take<double>((size_t)B * a.nblk);
    a.stats = c.take<double>((size_t)B * P3D_FULL_STATS);
    a.fixv = c.take<float>(slots);
    a.cnt = c.take<int>(slots + B);
    r.per_rep = c.take<double>((size_t)B * r.n_rep);
}
std::vector<int> full_meta(const int* n_fix, int n_maps, int n_rep, long long n_pix, size_t& n_idx) {
    std::vector<int> meta((size_t)n_maps * 3);
    long long slot = 0, idx = 0;
    for (int b = 0; b < n_maps; ++b) {
        if (n_fix[b] < 0 || n_fix[b] > n_pix) throw P3dError("n_fix out of range");
        meta[b * 3 + 0] = n_fix[b];
        meta[b * 3 + 1] = (int)slot;
        meta[b * 3 + 2] = (int)idx;
        slot += next_pow2(n_fix[b]);
        idx += (long long)n_fix[b] * n_rep;
        if (slot > INT32_MAX / 2 || idx > INT32_MAX) throw P3dError("too many fixations");
    }
    n_idx = (size_t)idx;
    return meta;
}
void check_indices(const int* idx, size_t n, long long n_pix, const char* what) {
    for (size_t i = 0; i < n; ++i)
        if (idx[i] < 0 || idx[i] >= n_pix) throw P3dError(std::string(what) + ": random index out of range");
}
// ---- the smoothing / normalisation stage of p3d_set_postprocess (postprocess.hip), one launch sequence for every caller ------
// What a setting asks for: the effective radius, its weights, the normalisation.  Built on the host, no HIP call.
struct PostPlan {
    bool on = false; int r = 0, norm = P3D_NORM_NONE; std::vector<float> taps;
    PostPlan() {}
    explicit PostPlan(const p3d_postprocess* cfg) {
        if (!cfg) return;
        r = p3d_handle::PostCfg::radius(*cfg);
        norm = cfg->norm;
        on = !p3d_handle::PostCfg::neutral(*cfg);
        if (r > 0) taps = p3d_handle::PostCfg::taps(cfg->sigma, r);
    }
    void fits(int H, int W) const {
        if (r > std::min(H, W) - 1)
            throw P3dError("postprocess: radius " + std::to_string(r) + " exceeds min(H, W) - 1 = " + std::to_string(std::min(H, W) - 1));
    }
};
using MatchPlan = p3d_handle::MatchCfg;
// p3d_set_prior_stage's stage for one launch sequence: the mode, the weight and the prior map (device memory) with its size
struct PriorStage {
    int mode = P3D_PRIOR_OFF; float a = 0.f; const float* map = nullptr; int H = 0, W = 0;
    bool on() const { return mode != P3D_PRIOR_OFF; }
    // refused when the stage runs: no prior, or a prior of another size than the stage's
    void fits(int sH, int sW) const {
        if (!on()) return;
        if (!map) throw P3dError("prior_stage: the handle has no prior (p3d_prior_finish or p3d_set_prior_map)");
        if (H != sH || W != sW)
            throw P3dError("prior_stage: the prior is " + std::to_string(H) + " x " + std::to_string(W) + ", the maps " + std::to_string(sH) + " x " + std::to_string(sW));
    }
};
// The stages of one launch sequence between the resize and the read-out: p3d_set_postprocess's blur and normalisation,
// p3d_set_prior_stage's stage after the blur, p3d_set_hist_match's matching after that and before the normalisation.
struct Stages {
    PostPlan post; MatchPlan match; PriorStage prior;
    Stages() {}
    // the handle's settings (each was parsed when it was set)
    explicit Stages(const p3d_handle* h)
        : post(h->post.on ? &h->post.cfg : nullptr), match(h->match), prior{h->prior.mode, h->prior.a, h->prior.map, h->prior.H, h->prior.W} {}
    // a hook's arguments, refused in this order: cfg, match.  prior: H x W floats, or null until the hook has its copy on the device
    Stages(const p3d_postprocess* cfg, const p3d_hist_match* m, const float* prior_, int mode, float a, int H, int W)
        : post(cfg), match(p3d_handle::MatchCfg::parse(m)), prior{mode, a, prior_, H, W} {}
    bool chain() const { return post.on || match.on() || prior.on(); }
    void fits(int H, int W) const { post.fits(H, W); prior.fits(H, W); }
};
// Device scratch of the stages for `chunk` maps of N pixels at a time
struct StageScratch {
    struct Post { float* maps = nullptr; float* tmp = nullptr; float* taps = nullptr; float* part = nullptr; float* mnmx = nullptr; } post;
    struct Match {
        float* part = nullptr; float* mnmx = nullptr; int* cnt = nullptr; double* cdf = nullptr; double* centre = nullptr; double* newv = nullptr;
        double* tcdf = nullptr; double* tcentre = nullptr;      // TABLE: the uploaded table; DENSITY: the targets' tables [chunk][nb]
        float* tpart = nullptr; float* tmnmx = nullptr;         // DENSITY: the targets' min / max
    } match;
    // own_maps: the maps live here too (no float32 output)
    void carve(Carve& c, const Stages& st, int chunk, long long N, bool own_maps) {
        const PostPlan& pl = st.post;
        post.maps = own_maps ? c.take<float>((size_t)chunk * N) : nullptr;
        post.tmp = pl.r > 0 ? c.take<float>((size_t)chunk * N) : nullptr;
        post.taps = pl.r > 0 ? c.take<float>((size_t)2 * pl.r + 1) : nullptr;
        post.part = pl.norm != P3D_NORM_NONE ? c.take<float>((size_t)chunk * p3d_post_blocks(N) * 2) : nullptr;
        post.mnmx = pl.norm != P3D_NORM_NONE ? c.take<float>((size_t)chunk * 2) : nullptr;
        const MatchPlan& mp = st.match;
        if (!mp.on()) return;
        const size_t k = (size_t)chunk * mp.nb;
        const bool dens = mp.mode == P3D_MATCH_DENSITY;
        match.part = c.take<float>((size_t)chunk * p3d_post_blocks(N) * 2);
        match.mnmx = c.take<float>((size_t)chunk * 2);
        match.cnt = c.take<int>(k);
        match.cdf = c.take<double>(k); match.centre = c.take<double>(k); match.newv = c.take<double>(k);
        match.tcdf = c.take<double>(dens ? k : mp.cdf.size());
        match.tcentre = c.take<double>(dens ? k : mp.centres.size());
        match.tpart = dens ? c.take<float>((size_t)chunk * p3d_post_blocks(N) * 2) : nullptr;
        match.tmnmx = dens ? c.take<float>((size_t)chunk * 2) : nullptr;
    }
};
// n maps of one source: map m's pixel (y, x) at p[m * map_stride + (y * w + x) * elem_stride] (device memory)
struct PostRun { const float* p; long long map_stride; int elem_stride, n; };
// One pass of `total` maps through the stages.  runs: the sources of h x w pixels, resized (float32) to H x W -- their n add up to
// total; empty: f32 already holds the maps.  f32 [total][H][W] (device) receives the float32 result, or null: the maps pass through
// the scratch's own.  u8 (device, 4-byte aligned) or null: map k's bytes, v * scale saturated, at u8_off + k * H * W.  density
// [total][H][W] (device): under P3D_MATCH_DENSITY map k's target, evaluation's float32(b / 255.) density.
struct PostJob {
    std::vector<PostRun> runs; int total = 0, h = 0, w = 0, H = 0, W = 0;
    float* f32 = nullptr; unsigned char* u8 = nullptr; long long u8_off = 0; float scale = 0.f;
    const float* density = nullptr;
};
// resize -> blur -> prior -> match -> normalise (-> quantise) of a job's maps on stream s, at most `chunk` maps per pass through the
// stages; a stage that is off is not issued.  counters: `chunk` zeroed arrival counters.  Queues only (after one synchronising
// upload of the taps and of a table).
void post_sequence(hipStream_t s, const Stages& st, const StageScratch& sc, unsigned* counters, int chunk, const PostJob& job) {
    const PostPlan& pl = st.post;
    const MatchPlan& mp = st.match;
    const StageScratch::Post& ps = sc.post;
    const StageScratch::Match& ms = sc.match;
    const int H = job.H, W = job.W, total = job.total;
    const std::vector<PostRun>& runs = job.runs;
    st.fits(H, W);
    const long long N = (long long)H * W;
    if (pl.r > 0) HIPCHECK(copy_now(ps.taps, pl.taps.data(), pl.taps.size() * sizeof(float), hipMemcpyHostToDevice, s));
    const bool match = mp.on();
    if (match && mp.mode == P3D_MATCH_DENSITY && !job.density) throw P3dError("hist_match: P3D_MATCH_DENSITY needs a ground-truth density (evaluation only)");
    if (match && mp.mode == P3D_MATCH_TABLE) {
        HIPCHECK(copy_now(ms.tcdf, mp.cdf.data(), mp.cdf.size() * sizeof(double), hipMemcpyHostToDevice, s));
        HIPCHECK(copy_now(ms.tcentre, mp.centres.data(), mp.centres.size() * sizeof(double), hipMemcpyHostToDevice, s));
    }
    size_t ri = 0;
    int rdone = 0;
    for (int done = 0; done < total; done += chunk) {
        const int cn = std::min(chunk, total - done);
        float* maps = job.f32 ? job.f32 + (size_t)done * N : ps.maps;
        for (int filled = 0; filled < cn && !runs.empty();) {
            while (runs[ri].n == rdone) { ++ri; rdone = 0; }
            const PostRun& R = runs[ri];
            const int take = std::min(R.n - rdone, cn - filled);
            PostArgs a;
            a.src = R.p + (size_t)rdone * R.map_stride; a.map_stride = R.map_stride; a.elem_stride = R.elem_stride; a.h = job.h; a.w = job.w;
            a.n = take; a.H = H; a.W = W; a.maps = maps + (size_t)filled * N;
            HIPCHECK(p3d_post_launch(POST_RESIZE, a, s));
            filled += take; rdone += take;
        }
        PostArgs a;
        a.n = cn; a.H = H; a.W = W; a.maps = maps; a.tmp = ps.tmp; a.taps = ps.taps; a.r = pl.r; a.norm = pl.norm;
        a.part = ps.part; a.mnmx = ps.mnmx; a.counter = counters; a.nblk = p3d_post_blocks(N);
        a.u8 = job.u8; a.u8_off = job.u8_off + (long long)done * N; a.scale = job.scale;
        if (st.prior.on()) { a.prior = st.prior.map; a.prior_mode = st.prior.mode; a.prior_a = st.prior.a; a.prior_b = (float)(1.0 - (double)st.prior.a); }
        HistChain hc;
        if (match) {
            HistArgs& q = hc.source;           // (its maps are a's: p3d_post_launch fills them in)
            q.nb = mp.nb; q.part = ms.part; q.mnmx = ms.mnmx; q.counter = counters; q.nblk = p3d_post_blocks(N);
            q.cnt = ms.cnt; q.cdf = ms.cdf; q.centre = ms.centre; q.newv = ms.newv; q.tcdf = ms.tcdf; q.tcentre = ms.tcentre;
            q.nt = mp.mode == P3D_MATCH_DENSITY ? mp.nb : (int)mp.cdf.size();
            q.t_stride = mp.mode == P3D_MATCH_DENSITY ? mp.nb : 0;
            if (mp.mode == P3D_MATCH_DENSITY) {
                HistArgs& t = hc.target;
                hc.has_target = true;
                t.maps = job.density + (size_t)done * N; t.kind = HIST_DENSITY; t.n = cn; t.H = H; t.W = W; t.nb = mp.nb;
                t.part = ms.tpart; t.mnmx = ms.tmnmx; t.counter = counters; t.nblk = q.nblk;
                t.cnt = ms.cnt; t.cdf = ms.tcdf; t.centre = ms.tcentre;      // (the integer tables are zeroed before every count)
            }
            a.match = &hc;
        }
        for (int st_i = POST_BLUR_H; st_i < POST_STAGES; ++st_i) HIPCHECK(p3d_post_launch(st_i, a, s));
    }
}
// Source maps of one evaluation: map m's pixel (y, x) at p[m * map_stride + (y * w + x) * elem_stride] (device memory)
struct EvalSource { const float* p; long long map_stride; int elem_stride, n_maps, h, w; };
// p3d_set_eval_extra's launch for one evaluation: the flags, the baseline of H x W floats and its statistics (device memory, IG
// only), and where the [n_maps][2] values go on the host
static_assert(P3D_EVAL_KLDIV == P3D_EXTRA_KLDIV && P3D_EVAL_INFO_GAIN == P3D_EXTRA_INFO_GAIN, "p3d_kernels.h names the header's flags");
struct EvalExtra { int flags; const float* base; const double* bstat; int H, W; double* out; };
// p3d_eval_shuffled_*'s part of one evaluation: the union of every clip's other fixations with its scan (device memory, fixpool.hip),
// the counts on the host, the pool's size, the host's ranks [n_rows[b]][n_rep] per clip, and where the [n_maps][n_rep] areas and the
// two HIP-event times (select; clean moments + borji) go on the host
struct ShuffledEval {
    const unsigned long long* uni; const unsigned* prefix; const unsigned* bsum; const unsigned* n_other_dev; const unsigned* n_other;
    long long nw; int H, W; const int* ranks; const int* n_rows; int n_rep; double step; double* per_rep; double* ms;
};
// What every evaluation is given, on the host: density uint8 [n_maps][Hd][Wd]; fixation uint8 [n_maps][H][W]; jitter (or null)
// float64 [n_maps][H][W]; AUC_Borji's draws borji_idx for n_fix [n_maps] fixations, n_rep and step_size; out [n_maps][5]
struct EvalInputs {
    const unsigned char* density; int Hd, Wd; const unsigned char* fixation; int H, W; const double* jitter;
    const int* borji_idx; const int* n_fix; int n_rep; double step_size; double* out;
};
// One evaluation.  src: the source maps; prepare (or empty) queues whatever makes them readable -- it runs after the uploads,
// inside the metric stage's time.  stage_ms (or null): the HIP-event times of the uploads and of the device pass.  extra, sh: null
// when off.
struct EvalRequest {
    EvalSource src{};
    std::function<void(hipStream_t)> prepare;
    EvalInputs in{};
    double* stage_ms = nullptr;
    Stages stages;
    const EvalExtra* extra = nullptr;
    const ShuffledEval* sh = nullptr;
};
// The device pass of test.py's per-batch body on stream s, with the scratch of s: everything of p3d_eval_last_frames that does
// not need the handle, so that p3d_debug_eval_maps runs the same launches on maps of the caller's.  Checks the arguments, lays
// the buffers out in the stream's scratch, uploads, resizes the source maps (float32) and the density maps (uint8), runs the
// metric passes, reads out[n_maps][5] back and compares n_fix with the device's counts.
void eval_maps(hipStream_t s, const EvalRequest& rq) {
    const EvalSource& src = rq.src;
    const Stages& st = rq.stages;
    const MatchPlan& match = st.match;
    const EvalExtra* const extra = rq.extra;
    const ShuffledEval* const sh = rq.sh;
    const EvalInputs& in = rq.in;
    const int Hd = in.Hd, Wd = in.Wd, H = in.H, W = in.W, n_rep = in.n_rep;
    const int* const n_fix = in.n_fix;
    const double* const jitter = in.jitter;
    const bool chain = st.chain();
    if (!src.p || !in.density || !in.fixation || !n_fix || !in.out) throw P3dError("null argument");
    if (Hd < 1 || Wd < 1 || H < 1 || W < 1) throw P3dError("eval: empty map");
    if ((long long)H * W > INT32_MAX / 2) throw P3dError("eval: map too large");
    if (n_rep < 1 || !(in.step_size > 0.0)) throw P3dError("eval: AUC_Borji needs n_rep >= 1 and a positive step");
    st.fits(H, W);
    const bool xon = extra && extra->flags != 0;                 // p3d_set_eval_extra: one launch after pass A, on the scored map
    if (xon && !extra->out) throw P3dError("null argument");
    if (xon && (extra->flags & P3D_EVAL_INFO_GAIN) && (!extra->base || !extra->bstat || extra->H != H || extra->W != W))
        throw P3dError("eval_extra: the baseline is " + std::to_string(extra->H) + " x " + std::to_string(extra->W) + ", the evaluation " +
                       std::to_string(H) + " x " + std::to_string(W));
    const int B = src.n_maps;
    const long long N = (long long)H * W;
    size_t n_idx = 0;
    const std::vector<int> meta = full_meta(n_fix, B, n_rep, N, n_idx);
    if (n_idx > 0 && !in.borji_idx) throw P3dError("eval: null random indices");
    check_indices(in.borji_idx, n_idx, N, "eval");
    // shuffled AUC (p3d_eval_shuffled_draws armed it): a second, clean P3dFullMaps on the same P with rows of its own per map
    std::vector<int> meta2;
    size_t n_idx2 = 0;
    int max_rows = 0;
    if (sh) {
        if (sh->H != H || sh->W != W)
            throw P3dError("eval_shuffled: the fixation pool is " + std::to_string(sh->H) + " x " + std::to_string(sh->W) + ", the evaluation " +
                           std::to_string(H) + " x " + std::to_string(W));
        if (!sh->per_rep) throw P3dError("null argument");
        p3d_handle::FixPool::check_draws("eval_shuffled", sh->ranks, sh->n_rows, sh->n_other, B, sh->n_rep, sh->step);
        for (int b = 0; b < B; ++b) {
            const long long want = std::min<long long>(n_fix[b], sh->n_other[b]);
            if (sh->n_rows[b] != want)
                throw P3dError("eval_shuffled: clip " + std::to_string(b) + ": " + std::to_string(sh->n_rows[b]) + " rows of ranks, but min(n_fix, n_other) = " +
                               std::to_string(want));
            max_rows = std::max(max_rows, sh->n_rows[b]);
        }
        meta2 = full_meta(n_fix, B, 0, N, n_idx2);
        long long at = 0;
        for (int b = 0; b < B; ++b) { meta2[b * 3 + 2] = (int)at; at += (long long)sh->n_rows[b] * sh->n_rep; }
        n_idx2 = (size_t)at;
    }
    P3dFullMaps a, a2;
    P3dFullBorji r, r2;
    int *ranks2 = nullptr, *idx2 = nullptr, *rows2 = nullptr;
    a.fix_u8 = 1; a.n_pix = N; a.n_maps = B; a.nblk = p3d_full_blocks(N); a.out = nullptr;
    r.n_rand = -1; r.n_rep = n_rep; r.step = in.step_size;
    if (sh) {
        a2.fix_u8 = 1; a2.n_pix = N; a2.n_maps = B; a2.nblk = a.nblk; a2.out = nullptr;
        r2.n_rep = sh->n_rep; r2.step = sh->step;
    }
    float *P = nullptr, *D = nullptr;
    unsigned char *dens = nullptr, *fixd = nullptr;
    double *jit = nullptr, *dout = nullptr;
    int* idx = nullptr;
    StageScratch scratch;
    P3dFullExtra x;
    const int post_chunk = std::min(B, P3D_POST_CHUNK);
    unsigned* const counters = carve_scratch(s, (size_t)B, [&](Carve& c) {
        P = c.take<float>((size_t)B * N);
        D = c.take<float>((size_t)B * N);
        dens = c.take<unsigned char>((size_t)B * Hd * Wd);
        fixd = c.take<unsigned char>((size_t)B * N);
        jit = c.take<double>(jitter ? (size_t)B * N : 0);
        idx = c.take<int>(n_idx);
        dout = c.take<double>((size_t)B * 5);
        carve_full(c, a, r, meta);
        scratch.carve(c, st, post_chunk, N, false);
        if (xon) { x.part = c.take<double>((size_t)B * a.nblk * P3D_FULL_EXTRA_PARTS); x.out = c.take<double>((size_t)B * 2); }
        if (sh) {
            ranks2 = c.take<int>(n_idx2); idx2 = c.take<int>(n_idx2); rows2 = c.take<int>((size_t)B);
            carve_full(c, a2, r2, meta2);
        }
    });
    a.P = P; a.D = D; a.fix = fixd; a.jit = jitter ? jit : nullptr; a.counter = counters; a.out = dout; r.idx = idx;
    if (sh) { a2.P = P; a2.fix = fixd; a2.counter = counters; r2.idx = idx2; r2.n_rand_map = rows2; }

    StageTimer tm(rq.stage_ms != nullptr, 3);
    tm.mark(0, s);
    HIPCHECK(copy_now(dens, in.density, (size_t)B * Hd * Wd, hipMemcpyHostToDevice, s));
    HIPCHECK(copy_now(fixd, in.fixation, (size_t)B * N, hipMemcpyHostToDevice, s));
    if (jitter) HIPCHECK(copy_now(jit, jitter, (size_t)B * N * sizeof(double), hipMemcpyHostToDevice, s));
    if (n_idx) HIPCHECK(copy_now(idx, in.borji_idx, n_idx * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHECK(copy_now((void*)a.meta, meta.data(), meta.size() * sizeof(int), hipMemcpyHostToDevice, s));
    tm.mark(1, s);
    if (rq.prepare) rq.prepare(s);
    const bool density_first = match.mode == P3D_MATCH_DENSITY;              // the stage reads D: the same launch, issued earlier
    if (density_first) HIPCHECK(p3d_mapf_density(dens, B, Hd, Wd, D, H, W, s));
    if (chain) {
        PostJob job;
        job.runs = {{src.p, src.map_stride, src.elem_stride, B}};
        job.total = B; job.h = src.h; job.w = src.w; job.H = H; job.W = W; job.f32 = P; job.density = D;
        post_sequence(s, st, scratch, counters, post_chunk, job);
    } else
        HIPCHECK(p3d_resize_f32(src.p, src.map_stride, src.elem_stride, B, src.h, src.w, P, H, W, s));
    if (!density_first) HIPCHECK(p3d_mapf_density(dens, B, Hd, Wd, D, H, W, s));      // test.py's density: uint8 resize (dataflow.py:236-238)
    HIPCHECK(p3d_full_moments(a, s));
    if (xon) {
        x.flags = extra->flags; x.base = extra->base; x.bstat = extra->bstat;
        HIPCHECK(p3d_full_extra(a, x, s));
    }
    HIPCHECK(p3d_full_rank(a, s));
    HIPCHECK(p3d_full_borji(a, r, s));
    if (sh) {                                  // after every launch of the plain evaluation: select, then the clean map's moments and borji
        if (n_idx2) HIPCHECK(copy_now(ranks2, sh->ranks, n_idx2 * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHECK(copy_now(rows2, sh->n_rows, (size_t)B * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHECK(copy_now((void*)a2.meta, meta2.data(), meta2.size() * sizeof(int), hipMemcpyHostToDevice, s));
        StageTimer t2(true, 3);
        t2.mark(0, s);
        if (n_idx2) {
            FixSelectArgs q;
            q.uni = sh->uni; q.prefix = sh->prefix; q.bsum = sh->bsum; q.n_other = sh->n_other_dev; q.nw = sh->nw; q.B = B;
            q.nsb = p3d_fix_scan_blocks(sh->nw); q.n_rep = sh->n_rep; q.max_rows = max_rows; q.meta = a2.meta; q.n_rows = rows2; q.ranks = ranks2;
            q.out = idx2;
            HIPCHECK(p3d_fix_select_launch(q, s));
        }
        t2.mark(1, s);
        HIPCHECK(p3d_full_moments(a2, s));
        HIPCHECK(p3d_full_borji(a2, r2, s));
        t2.mark(2, s);
        HIPCHECK(copy_now(sh->per_rep, r2.per_rep, (size_t)B * sh->n_rep * sizeof(double), hipMemcpyDeviceToHost, s));
        const float t0 = t2.ms(0), t1 = t2.ms(1);
        if (sh->ms) { sh->ms[0] = t0; sh->ms[1] = t1; }
    }
    tm.mark(2, s);
    std::vector<double> stats((size_t)B * P3D_FULL_STATS);
    HIPCHECK(copy_now(in.out, dout, (size_t)B * 5 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (xon) HIPCHECK(copy_now(extra->out, x.out, (size_t)B * 2 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHECK(copy_now(stats.data(), a.stats, stats.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    if (rq.stage_ms) { rq.stage_ms[0] = tm.ms(0); rq.stage_ms[1] = tm.ms(1); }
    for (int b = 0; b < B; ++b)
        if ((long long)stats[(size_t)b * P3D_FULL_STATS + P3D_FULL_STAT_NFIX] != n_fix[b])
            throw P3dError("eval: clip " + std::to_string(b) + ": n_fix = " + std::to_string(n_fix[b]) + " but its fixation map has " +
                           std::to_string((long long)stats[(size_t)b * P3D_FULL_STATS + P3D_FULL_STAT_NFIX]) + " fixated pixels");
}
}  // namespace
extern "C" {

int p3d_resize_linear(int device, const float* src, int n, int h, int w, int H, int W, float* dst) {
    API_BEGIN
    metric_args(device, src, src, 1, 1, dst);
    if (n < 1 || h < 1 || w < 1 || H < 1 || W < 1) throw P3dError("resize: empty map");
    DevArr<float> s((size_t)n * h * w, src), d((size_t)n * H * W);
    HIPCHECK(p3d_resize_f32(s.p, (long long)h * w, 1, n, h, w, d.p, H, W, nullptr));
    d.get(dst, (size_t)n * H * W);
    API_END
}

int p3d_metric_auc_shuffled(int device, const float* sal, const float* fix, const int* other_idx, int n_pix, int n_fix, int n_rand,
                            int n_rep, double step_size, double* out) {
    API_BEGIN
    metric_args(device, sal, fix, 1, n_pix, out);
    if (n_rep < 1 || !(step_size > 0.0)) throw P3dError("AUC_shuffled needs n_rep >= 1 and a positive step");
    if (n_rand < 0 || n_rand > n_fix) throw P3dError("AUC_shuffled: n_rand must be in [0, n_fix]");
    if (n_rand > 0 && !other_idx) throw P3dError("AUC_shuffled: null random indices");
    check_indices(other_idx, (size_t)n_rand * n_rep, n_pix, "AUC_shuffled");
    P3dFullMaps a;
    P3dFullBorji r;
    a.fix = nullptr; a.fix_u8 = 0; a.n_pix = n_pix; a.n_maps = 1; a.nblk = p3d_full_blocks(n_pix);
    r.n_rand = n_rand; r.n_rep = n_rep; r.step = step_size;
    size_t n_idx = 0;
    const std::vector<int> meta = full_meta(&n_fix, 1, 0, n_pix, n_idx);
    Carve c;
    carve_full(c, a, r, meta);
    DevArr<char> scratch(c.off);
    c = Carve{scratch.p, 0};
    carve_full(c, a, r, meta);
    DevArr<float> dsal(n_pix, sal), dfix(n_pix, fix);
    DevArr<int> didx((size_t)n_rand * n_rep, other_idx);
    const unsigned zero = 0;
    DevArr<unsigned> counter(1, &zero);
    HIPCHECK(copy_now((void*)a.meta, meta.data(), meta.size() * sizeof(int), hipMemcpyHostToDevice, nullptr));
    a.P = dsal.p; a.fix = dfix.p; a.counter = counter.p; r.idx = didx.p;
    HIPCHECK(p3d_full_moments(a, nullptr));
    double st[P3D_FULL_STATS];
    HIPCHECK(copy_now(st, a.stats, sizeof(st), hipMemcpyDeviceToHost, nullptr));
    HIPCHECK(hipDeviceSynchronize());
    if ((int)st[P3D_FULL_STAT_NFIX] != n_fix)
        throw P3dError("AUC_shuffled: n_fix = " + std::to_string(n_fix) + " but the fixation map has " +
                       std::to_string((long long)st[P3D_FULL_STAT_NFIX]) + " fixated pixels");
    if (n_fix == 0) { for (int i = 0; i < n_rep; ++i) out[i] = NAN; return 0; }      // "no fixation to predict"
    HIPCHECK(p3d_full_borji(a, r, nullptr));
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(copy_now(out, r.per_rep, (size_t)n_rep * sizeof(double), hipMemcpyDeviceToHost, nullptr));
    HIPCHECK(hipDeviceSynchronize());
    API_END
}

int p3d_eval_last_frames(p3d_handle* h, const unsigned char* density, int Hd, int Wd, const unsigned char* fixation, int H, int W,
                         const double* jitter, const int* borji_idx, const int* n_fix, int n_rep, double step_size, double* out,
                         double* stage_ms) {
    API_BEGIN
    if (!h) throw P3dError("null argument");
    HIPCHECK(hipSetDevice(h->cfg.device));
    // the prediction of the last forward pass, frame T-1 of every clip: [B][T][h][w] with an element stride of ld floats
    Act* pr = h->pred;
    const int T = pr->D;
    const long long hw = (long long)pr->H * pr->W;
    EvalRequest rq;
    rq.src = {pr->p + (size_t)(T - 1) * hw * pr->ld, (long long)T * hw * pr->ld, pr->ld, pr->N, pr->H, pr->W};
    if (pr->materialize && h->last_forward_fused) rq.prepare = pr->materialize;
    rq.in = {density, Hd, Wd, fixation, H, W, jitter, borji_idx, n_fix, n_rep, step_size, out};
    rq.stage_ms = stage_ms;
    rq.stages = Stages(h);
    // p3d_set_eval_extra: its launch joins the sequence; an evaluation of another size than the baseline's runs without it and
    // p3d_last_eval_extra says so
    EvalExtra extra{h->extra.flags, h->extra.base, h->extra.bstat, h->extra.H, h->extra.W, nullptr};
    const bool fits = !(extra.flags & P3D_EVAL_INFO_GAIN) || (extra.H == H && extra.W == W);
    std::vector<double> xv((size_t)pr->N * 2);
    extra.out = xv.data();
    if (extra.flags) { h->extra.state = p3d_handle::EXTRA_NONE; h->extra.eval_H = H; h->extra.eval_W = W; }
    // p3d_eval_shuffled_draws armed this one evaluation: whatever becomes of it, the next one is plain again
    const bool armed = h->fixpool.armed;
    h->fixpool.armed = false;
    std::vector<double> sv;
    ShuffledEval sh{};
    if (armed) {
        if ((int)h->fixpool.sh.n_other.size() != pr->N) throw P3dError("eval_shuffled: the union was taken for " + std::to_string(h->fixpool.sh.n_other.size()) + " clips, the batch has " + std::to_string(pr->N));
        sv.assign((size_t)pr->N * h->fixpool.n_rep, 0.0);
        h->fixpool.have = false;
        sh = ShuffledEval{h->fixpool.sh.uni, h->fixpool.sh.prefix, h->fixpool.sh.bsum, h->fixpool.sh.n_other_dev, h->fixpool.sh.n_other.data(), h->fixpool.nw, h->fixpool.H, h->fixpool.W,
                          h->fixpool.ranks.data(), h->fixpool.n_rows.data(), h->fixpool.n_rep, h->fixpool.step, sv.data(), h->fixpool_ms + 2};
    }
    rq.extra = extra.flags && fits ? &extra : nullptr;
    rq.sh = armed ? &sh : nullptr;
    eval_maps(h->stream, rq);
    if (armed) { h->fixpool.last.swap(sv); h->fixpool.have = true; }
    if (extra.flags) {
        h->extra.state = fits ? p3d_handle::EXTRA_HAVE : p3d_handle::EXTRA_SHAPE;
        if (fits) h->extra.last.swap(xv);
    }
    API_END
}

// ---- p3d_set_eval_extra: KL divergence and information gain (full_pass_kl, metrics_full.hip) -----------------------------------
int p3d_set_eval_extra(p3d_handle* h, int flags, const float* baseline, int H, int W) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->set_eval_extra(flags, baseline, H, W);
    API_END
}

int p3d_get_eval_extra(p3d_handle* h, int* flags, const float** baseline, int* H, int* W) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    if (flags) *flags = h->extra.flags;
    if (baseline) *baseline = h->extra.base_host.empty() ? nullptr : h->extra.base_host.data();
    if (H) *H = h->extra.H;
    if (W) *W = h->extra.W;
    API_END
}

int p3d_last_eval_extra(p3d_handle* h, double* out, int64_t cap) {
    API_BEGIN
    if (!h || !out) throw P3dError("null argument");
    if (!h->extra.flags) throw P3dError("last_eval_extra: the option is off (p3d_set_eval_extra)");
    if (h->extra.state == p3d_handle::EXTRA_SHAPE)
        throw P3dError("last_eval_extra: the baseline is " + std::to_string(h->extra.H) + " x " + std::to_string(h->extra.W) +
                       ", the last evaluation scored " + std::to_string(h->extra.eval_H) + " x " + std::to_string(h->extra.eval_W) + " maps");
    if (h->extra.state != p3d_handle::EXTRA_HAVE) throw P3dError("last_eval_extra: no evaluation has run since the option was set");
    if (cap < (int64_t)h->extra.last.size())
        throw P3dError("last_eval_extra: room for " + std::to_string(cap) + " doubles, " + std::to_string(h->extra.last.size()) + " needed");
    std::copy(h->extra.last.begin(), h->extra.last.end(), out);
    API_END
}

}  // extern "C"
namespace {
// op level: the statistics of n maps by full_stats3 (private scratch), then full_pass_kl with them
struct Stats3 {
    DevArr<double> part, out; DevArr<unsigned> counter;
    Stats3(int n, long long N) : part((size_t)n * p3d_full_blocks(N) * P3D_FULL_STATS3_PARTS), out((size_t)n * 3),
                                 counter((size_t)n, std::vector<unsigned>((size_t)n, 0u).data()) {}
    void run(const float* maps, int n, long long N) {
        P3dFullStats3 q;
        q.maps = maps; q.n_pix = N; q.n_maps = n; q.nblk = p3d_full_blocks(N); q.part = part.p; q.counter = counter.p; q.out = out.p;
        HIPCHECK(p3d_full_stats3(q, nullptr));
    }
};
void metric_extra(int device, int flags, const float* map1, const float* map2, const float* baseline, int n_maps, int n_pix, double* out) {
    metric_args(device, map1, map2, n_maps, n_pix, out);
    if (n_maps > 65535) throw P3dError("at most 65535 maps per call");
    const bool ig = flags == P3D_EVAL_INFO_GAIN;
    if (ig) p3d_handle::Extra::check(flags, baseline, 1, n_pix);
    const size_t n = (size_t)n_maps * n_pix;
    DevArr<float> d1(n, map1), d2(n, map2), base(ig ? n_pix : 1, ig ? baseline : nullptr);
    Stats3 s1(n_maps, n_pix), s2(n_maps, n_pix), sb(1, n_pix);
    s1.run(d1.p, n_maps, n_pix);
    if (ig) sb.run(base.p, 1, n_pix); else s2.run(d2.p, n_maps, n_pix);
    P3dFullMaps a;
    P3dFullExtra x;
    a.P = d1.p; a.n_pix = n_pix; a.n_maps = n_maps; a.nblk = p3d_full_blocks(n_pix); a.counter = s1.counter.p;
    if (ig) { a.fix = d2.p; a.fix_u8 = 0; x.base = base.p; x.bstat = sb.out.p; } else { a.D = d2.p; x.ystat = s2.out.p; }
    DevArr<double> part((size_t)n_maps * a.nblk * P3D_FULL_EXTRA_PARTS), res((size_t)n_maps * 2);
    x.flags = flags; x.sstat = s1.out.p; x.part = part.p; x.out = res.p;
    HIPCHECK(p3d_full_extra(a, x, nullptr));
    std::vector<double> both((size_t)n_maps * 2);
    res.get(both.data(), both.size());
    for (int b = 0; b < n_maps; ++b) out[b] = both[(size_t)b * 2 + (ig ? 1 : 0)];
}
}  // namespace
extern "C" {

int p3d_metric_kldiv(int device, const float* map1, const float* map2, int n_maps, int n_pix, double* out) {
    API_BEGIN
    metric_extra(device, P3D_EVAL_KLDIV, map1, map2, nullptr, n_maps, n_pix, out);
    API_END
}

int p3d_metric_info_gain(int device, const float* sal, const float* fix, const float* baseline, int n_maps, int n_pix, double* out) {
    API_BEGIN
    if (!baseline) throw P3dError("null argument");
    metric_extra(device, P3D_EVAL_INFO_GAIN, sal, fix, baseline, n_maps, n_pix, out);
    API_END
}

int p3d_resize_linear_u8(int device, const float* src, int n, int h, int w, float scale, int H, int W, unsigned char* dst) {
    API_BEGIN
    metric_args(device, src, src, 1, 1, dst);
    if (n < 1 || h < 1 || w < 1 || H < 1 || W < 1) throw P3dError("resize_u8: empty map");
    if ((long long)H * W > INT32_MAX) throw P3dError("resize_u8: H * W exceeds the kernel's int32 in-map offsets");
    DevArr<float> s((size_t)n * h * w, src);
    DevArr<unsigned char> d((size_t)n * H * W);
    HIPCHECK(p3d_resize_u8(s.p, (long long)h * w, 1, n, h, w, scale, d.p, 0, H, W, nullptr));
    d.get(dst, (size_t)n * H * W);
    API_END
}

}  // extern "C"
namespace {
// What runs behind n maps of H x W device bytes, at four moments: carve (its buffers, from a caller's scratch), upload, launch,
// results.  A constructor refuses what its request gets wrong and queues nothing.
struct ByteStage {
    const char* who; int n, H, W;
    size_t bytes; bool timed; double ms[3] = {0.0, 0.0, 0.0};
    template <typename Request>
    explicit ByteStage(const Request& r) : who(r.who), n(r.n), H(r.H), W(r.W), bytes((size_t)r.n * (size_t)r.H * (size_t)r.W), timed(r.timed) {}
    virtual ~ByteStage() = default;
    virtual size_t counters() const { return 0; }
    virtual void carve(Carve& c) = 0;
    virtual void upload(hipStream_t s) = 0;
    virtual void launch(hipStream_t s, const unsigned char* sal, unsigned* counters) = 0;
    virtual void results(hipStream_t s) = 0;
};
// A stage's optional shot table in frames of the call: the host's (shots_table_check has passed it) and its copy on the device
struct ShotTable {
    const int32_t* host = nullptr; int n = 0; int32_t* dev = nullptr;
    void carve(Carve& c) { dev = host ? c.input<int32_t>((size_t)n) : nullptr; }
    void upload(hipStream_t s) const { if (dev) HIPCHECK(hipMemcpyAsync(dev, host, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s)); }
    template <typename Args> void bind(Args& a) const { a.starts = dev; a.n_shots = dev ? n : 0; }
};
// gen_pred.py's write-out of `maps` maps that live on the device, for p3d_pred_maps_u8 and p3d_video_maps_u8: the bytes, the
// scratch of p3d_set_postprocess's stage and `extra` floats of the caller's share one slab of the stream's scratch.  sources runs
// inside the device stage's time: it queues whatever makes the maps readable and names them as runs of maps of ph x pw pixels.
// Off: one double-precision p3d_resize_u8 per run; on: the float32 resize / blur / normalise / byte sequence, P3D_POST_CHUNK maps
// at a time.  Ends synchronised; stage_ms as p3d_pred_maps_u8's.
// A stage (a ByteStage) takes the device bytes where they are instead of a copy of the chain: its buffers are carved
// after the chain's in the same layout, its upload is queued ahead of the sources, its launches behind the chain with the bytes
// and counters() zeroed arrival counters of its own (after the chain's), its results (the copies back to the host) behind that;
// out may then be NULL (the bytes stay on the device) and, timed, its ms [3] receives the times of the upload, of the device stage
// and of the launches.  Without one, nothing here differs from what p3d_pred_maps_u8 and p3d_video_maps_u8 issue.
void maps_u8_chain(p3d_handle* h, long long maps, int ph, int pw, float scale, int H, int W, unsigned char* out, double* stage_ms,
                   size_t extra, const std::function<void(hipStream_t, float*, std::vector<PostRun>&)>& sources,
                   ByteStage* stage = nullptr) {
    const long long hw = (long long)H * W, bytes = maps * hw;
    const hipStream_t s = h->stream;
    // p3d_set_postprocess: the float32 chain resize -> blur -> normalise -> bytes, P3D_POST_CHUNK maps at a time; its scratch
    // follows the bytes in the slab.  Off: the double-precision resize below, as before.
    // p3d_set_hist_match: a table takes the same float32 chain, with its stage after the blur; the density mode has no target here
    // p3d_set_prior_stage: the same float32 chain, with its stage after the blur
    const Stages st(h);
    st.post.fits(H, W);
    if (st.match.mode == P3D_MATCH_DENSITY)
        throw P3dError("hist_match: P3D_MATCH_DENSITY matches to a ground-truth density and runs in p3d_eval_last_frames only; written maps take P3D_MATCH_TABLE");
    st.prior.fits(H, W);
    const bool chain = st.chain();
    const int post_chunk = (int)std::min<long long>(maps, P3D_POST_CHUNK);
    StageScratch scratch;
    unsigned char* d = nullptr;
    float* ex = nullptr;
    const size_t chain_counters = chain ? (size_t)post_chunk : 0;
    unsigned* const counters = carve_scratch(s, chain_counters + (stage ? stage->counters() : 0), [&](Carve& c) {
        d = c.take<unsigned char>((size_t)bytes);      // (the first take starts at offset 0: with nothing else, the slab is the bytes)
        if (chain) scratch.carve(c, st, post_chunk, hw, true);
        ex = extra ? c.take<float>(extra) : nullptr;
        if (stage) stage->carve(c);
    });
    const bool timed = stage && stage->timed;
    StageTimer tm(stage_ms != nullptr || timed, 3), ends(timed, 2);
    ends.mark(0, s);
    if (stage) stage->upload(s);
    tm.mark(0, s);
    PostJob job;
    sources(s, ex, job.runs);
    if (chain) {
        job.total = (int)maps; job.h = ph; job.w = pw; job.H = H; job.W = W; job.u8 = d; job.scale = scale;
        post_sequence(s, st, scratch, counters, post_chunk, job);
    } else {
        long long off = 0;
        for (const PostRun& r : job.runs) {
            HIPCHECK(p3d_resize_u8(r.p, r.map_stride, r.elem_stride, r.n, ph, pw, scale, d, off, H, W, s));
            off += r.n * hw;
        }
    }
    tm.mark(1, s);
    if (stage) stage->launch(s, d, counters + chain_counters);
    ends.mark(1, s);
    if (stage) stage->results(s);
    if (out) HIPCHECK(hipMemcpyAsync(out, d, (size_t)bytes, hipMemcpyDeviceToHost, s));
    tm.mark(2, s);
    HIPCHECK(hipStreamSynchronize(s));
    if (stage_ms) { stage_ms[0] = tm.ms(0); stage_ms[1] = tm.ms(1); }
    if (timed) {
        float up = 0.f, sc = 0.f;
        HIPCHECK(hipEventElapsedTime(&up, ends.ev[0], tm.ev[0]));
        HIPCHECK(hipEventElapsedTime(&sc, tm.ev[1], ends.ev[1]));
        stage->ms[0] = (double)up; stage->ms[1] = tm.ms(0); stage->ms[2] = (double)sc;
    }
}
}  // namespace
extern "C" {

int p3d_pred_maps_u8(p3d_handle* h, const int* first_frame, float scale, int H, int W, unsigned char* out, double* stage_ms) {
    API_BEGIN
    if (!h || !first_frame || !out) throw P3dError("null argument");
    if (H < 1 || W < 1) throw P3dError("pred_maps_u8: empty map");
    if ((long long)H * W > INT32_MAX) throw P3dError("pred_maps_u8: H * W exceeds the kernel's int32 in-map offsets");
    if (!h->pred_ready) throw P3dError("pred_maps_u8: the handle has no prediction yet (run a forward pass first)");
    Act* pr = h->pred;
    const int B = pr->N, T = pr->D;
    long long maps = 0;
    for (int b = 0; b < B; ++b) {
        if (first_frame[b] < 0 || first_frame[b] > T)
            throw P3dError("pred_maps_u8: first_frame[" + std::to_string(b) + "] = " + std::to_string(first_frame[b]) +
                           " is outside [0, " + std::to_string(T) + "]");
        maps += T - first_frame[b];
    }
    if (stage_ms) stage_ms[0] = stage_ms[1] = 0.0;
    if (maps == 0) return 0;
    HIPCHECK(hipSetDevice(h->cfg.device));
    // the prediction of the last forward pass: [B][T][h][w] with an element stride of ld floats; clip b's frames
    // first_frame[b] .. T-1, packed after the maps of the clips before it
    maps_u8_chain(h, maps, pr->H, pr->W, scale, H, W, out, stage_ms, 0, [&](hipStream_t s, float*, std::vector<PostRun>& runs) {
        if (pr->materialize && h->last_forward_fused) pr->materialize(s);
        const long long phw = (long long)pr->H * pr->W;
        for (int b = 0; b < B; ++b) {
            const int f0 = first_frame[b], n = T - f0;
            if (n > 0) runs.push_back({pr->p + ((size_t)b * T + f0) * phw * pr->ld, phw * pr->ld, pr->ld, n});
        }
    });
    API_END
}

// ---- p3d_set_postprocess and the op-level entry points of its stage ----------------------------------------------------------
int p3d_set_postprocess(p3d_handle* h, const p3d_postprocess* cfg) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    h->set_postprocess(cfg);
    API_END
}

int p3d_get_postprocess(p3d_handle* h, p3d_postprocess* cfg, int* on) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    if (cfg) *cfg = h->post.cfg;
    if (on) *on = h->post.on ? 1 : 0;
    API_END
}

int p3d_blur_taps(float sigma, int radius, float* taps, int cap, int* r) {
    API_BEGIN
    const p3d_postprocess cfg{sigma, radius, P3D_NORM_NONE};
    const PostPlan plan(&cfg);
    if (plan.r > 0) {
        if (!taps || cap < 2 * plan.r + 1) throw P3dError("blur_taps: room for " + std::to_string(2 * plan.r + 1) + " floats is needed");
        memcpy(taps, plan.taps.data(), plan.taps.size() * sizeof(float));
    }
    if (r) *r = plan.r;
    API_END
}

int p3d_debug_blur_strip(int r, int* cols, int* rows, int* lds_bytes) {
    API_BEGIN
    if (r < 0 || r > P3D_BLUR_MAX_RADIUS || !cols || !rows || !lds_bytes) throw P3dError("blur_strip: radius in [0, 255] and three results");
    const PostStrip st = p3d_post_strip(r);
    *cols = st.cols; *rows = st.rows; *lds_bytes = st.lds_bytes;
    API_END
}

int p3d_gaussian_blur(int device, const float* src, int n, int H, int W, float sigma, int radius, float* dst) {
    API_BEGIN
    const p3d_postprocess cfg{sigma, radius, P3D_NORM_NONE};
    Stages st;
    st.post = PostPlan(&cfg);
    metric_args(device, src, src, 1, 1, dst);
    if (n < 1 || H < 1 || W < 1) throw P3dError("gaussian_blur: empty map");
    if ((long long)H * W > INT32_MAX) throw P3dError("gaussian_blur: H * W exceeds the kernels' int32 in-map offsets");
    st.post.fits(H, W);
    const long long N = (long long)H * W;
    const int chunk = std::min(n, P3D_POST_CHUNK);
    DevArr<float> maps((size_t)n * N, src);
    StageScratch scratch;
    unsigned* const counters = carve_scratch(nullptr, (size_t)chunk, [&](Carve& c) { scratch.carve(c, st, chunk, N, false); });
    PostJob job;
    job.total = n; job.h = H; job.w = W; job.H = H; job.W = W; job.f32 = maps.p;
    post_sequence(nullptr, st, scratch, counters, chunk, job);
    maps.get(dst, (size_t)n * N);
    API_END
}

}  // extern "C"
namespace {
// Everything p3d_postprocess_maps_prior takes; the two hooks below it leave the match and the prior off
struct PostHook {
    int device; const float* maps; int n, h, w, elem_stride, H, W; const p3d_postprocess* cfg; const p3d_hist_match* match;
    const float* prior; int mode; float a; float scale; float* out_f32; unsigned char* out_u8;
};
void postprocess_maps(const PostHook& q) {
    const int n = q.n, H = q.H, W = q.W;
    Stages st(q.cfg, q.match, nullptr, q.mode, q.a, H, W);
    p3d_handle::PriorMap::stage_check(q.mode, q.a);
    if (st.prior.on()) p3d_handle::PriorMap::check(q.prior, H, W);      // (the prior of the hook has the stage's size)
    if (st.match.mode == P3D_MATCH_DENSITY) throw P3dError("hist_match: P3D_MATCH_DENSITY runs in evaluation only; supplied maps take P3D_MATCH_TABLE");
    metric_args(q.device, q.maps, q.maps, 1, 1, q.maps);
    if (n < 1 || q.h < 1 || q.w < 1 || q.elem_stride < 1 || H < 1 || W < 1) throw P3dError("postprocess_maps: empty map");
    if ((long long)H * W > INT32_MAX) throw P3dError("postprocess_maps: H * W exceeds the kernels' int32 in-map offsets");
    st.post.fits(H, W);
    const long long N = (long long)H * W, per_map = (long long)q.h * q.w * q.elem_stride, ne = (long long)n * N;
    const int chunk = std::min(n, P3D_POST_CHUNK);
    DevArr<float> src((size_t)n * per_map, q.maps), dprior(st.prior.on() ? (size_t)N : 1, st.prior.on() ? q.prior : nullptr);
    st.prior.map = dprior.p;
    // the outputs between guards: 8 floats either side of out_f32; out_u8 at byte 19 of its buffer, so that the BYTE kernel's
    // unaligned head and tail run
    Guarded<float> fbuf(q.out_f32 ? (size_t)ne : 0, 8, 0, nullptr);
    Guarded<unsigned char> bbuf(q.out_u8 ? (size_t)ne : 0, 16, 3, nullptr);
    StageScratch scratch;
    unsigned* const counters = carve_scratch(nullptr, (size_t)chunk, [&](Carve& c) { scratch.carve(c, st, chunk, N, !q.out_f32); });
    PostJob job;
    job.runs = {{src.p, per_map, q.elem_stride, n}};
    job.total = n; job.h = q.h; job.w = q.w; job.H = H; job.W = W; job.scale = q.scale;
    job.f32 = q.out_f32 ? fbuf.data() : nullptr;
    job.u8 = q.out_u8 ? bbuf.dev.p : nullptr; job.u8_off = (long long)bbuf.at;
    post_sequence(nullptr, st, scratch, counters, chunk, job);
    if (q.out_f32) fbuf.back(q.out_f32, "postprocess_maps");
    if (q.out_u8) bbuf.back(q.out_u8, "postprocess_maps");
    if (!q.out_f32 && !q.out_u8) HIPCHECK(hipDeviceSynchronize());
}

// Device buffers of one op-level launch sequence of hist_match.hip on n maps (no stream scratch: private allocations)
struct HistBufs {
    DevArr<float> part, mnmx; DevArr<unsigned> counter; DevArr<int> cnt; DevArr<long long> counts; DevArr<double> cdf, centre, newv;
    static std::vector<unsigned> zeros(int n) { return std::vector<unsigned>((size_t)n, 0u); }
    HistBufs(int n, long long N, int nb)
        : part((size_t)n * p3d_post_blocks(N) * 2), mnmx((size_t)n * 2), counter((size_t)n, zeros(n).data()), cnt((size_t)n * nb),
          counts((size_t)n * nb), cdf((size_t)n * nb), centre((size_t)n * nb), newv((size_t)n * nb) {}
    HistArgs args(const float* maps, int n, int H, int W, int nb) {
        HistArgs a;
        a.maps = maps; a.n = n; a.H = H; a.W = W; a.nb = nb; a.part = part.p; a.mnmx = mnmx.p; a.counter = counter.p;
        a.nblk = p3d_post_blocks((long long)H * W); a.cnt = cnt.p; a.counts = counts.p; a.cdf = cdf.p; a.centre = centre.p; a.newv = newv.p;
        return a;
    }
};
void hist_shape(const char* what, const void* maps, const void* out, int n, int H, int W, int nbins) {
    p3d_handle::MatchCfg::bins(what, nbins);
    if (!maps || !out) throw P3dError(std::string(what) + ": null argument");
    if (n < 1 || n > 65535 || H < 1 || W < 1) throw P3dError(std::string(what) + ": 1 .. 65535 maps of at least one pixel");
    if ((long long)H * W > INT32_MAX) throw P3dError(std::string(what) + ": H * W exceeds the kernels' int32 in-map offsets");
}
}  // namespace
extern "C" {

int p3d_postprocess_maps(int device, const float* maps, int n, int h, int w, int elem_stride, int H, int W,
                         const p3d_postprocess* cfg, float scale, float* out_f32, unsigned char* out_u8) {
    API_BEGIN
    postprocess_maps({device, maps, n, h, w, elem_stride, H, W, cfg, nullptr, nullptr, P3D_PRIOR_OFF, 0.f, scale, out_f32, out_u8});
    API_END
}

int p3d_postprocess_maps_match(int device, const float* maps, int n, int h, int w, int elem_stride, int H, int W,
                               const p3d_postprocess* cfg, const p3d_hist_match* match, float scale, float* out_f32, unsigned char* out_u8) {
    API_BEGIN
    postprocess_maps({device, maps, n, h, w, elem_stride, H, W, cfg, match, nullptr, P3D_PRIOR_OFF, 0.f, scale, out_f32, out_u8});
    API_END
}

int p3d_postprocess_maps_prior(int device, const float* maps, int n, int h, int w, int elem_stride, int H, int W, const p3d_postprocess* cfg,
                               const p3d_hist_match* match, const float* prior, int mode, float a, float scale, float* out_f32,
                               unsigned char* out_u8) {
    API_BEGIN
    postprocess_maps({device, maps, n, h, w, elem_stride, H, W, cfg, match, prior, mode, a, scale, out_f32, out_u8});
    API_END
}

// ---- p3d_set_hist_match and the op-level entry points of its stage (hist_match.hip) ------------------------------------------
int p3d_set_hist_match(p3d_handle* h, const p3d_hist_match* cfg) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    h->set_hist_match(cfg);
    API_END
}

int p3d_get_hist_match(p3d_handle* h, p3d_hist_match* cfg) {
    API_BEGIN
    if (!h || !cfg) throw P3dError("null argument");
    const p3d_handle::MatchCfg& m = h->match;
    cfg->mode = m.mode; cfg->nbins = m.on() ? m.nb : 0; cfg->nt = (int)m.cdf.size();
    cfg->cdf = m.cdf.empty() ? nullptr : m.cdf.data();
    cfg->centres = m.centres.empty() ? nullptr : m.centres.data();
    API_END
}

int p3d_cumulative_distribution(int device, const float* maps, int n, int H, int W, int nbins, int64_t* counts, double* cdf, double* centres) {
    API_BEGIN
    hist_shape("cumulative_distribution", maps, cdf, n, H, W, nbins);
    if (!centres) throw P3dError("cumulative_distribution: null argument");
    metric_args(device, maps, maps, 1, 1, cdf);
    const long long N = (long long)H * W;
    DevArr<float> src((size_t)n * N, maps);
    HistBufs b(n, N, nbins);
    const HistArgs a = b.args(src.p, n, H, W, nbins);
    for (int st = 0; st < HIST_STAGES; ++st) HIPCHECK(p3d_hist_launch(st, a, nullptr));
    b.cdf.get(cdf, (size_t)n * nbins);
    b.centre.get(centres, (size_t)n * nbins);
    if (counts) {
        static_assert(sizeof(long long) == sizeof(int64_t), "counts are int64");
        b.counts.get(reinterpret_cast<long long*>(counts), (size_t)n * nbins);
    }
    API_END
}

int p3d_match_hist(int device, const float* maps, int n, int H, int W, int nbins, const double* cdf_t, const double* centre_t, int n_tables,
                   int nt, float* out) {
    API_BEGIN
    hist_shape("match_hist", maps, out, n, H, W, nbins);
    if (n_tables != 1 && n_tables != n) throw P3dError("match_hist: one table, or one per map");
    p3d_handle::MatchCfg::table("match_hist", cdf_t, centre_t, nt, n_tables);
    metric_args(device, maps, maps, 1, 1, out);
    const long long N = (long long)H * W;
    DevArr<float> src((size_t)n * N, maps), dst((size_t)n * N);
    DevArr<double> tc((size_t)n_tables * nt, cdf_t), tx((size_t)n_tables * nt, centre_t);
    HistBufs b(n, N, nbins);
    HistArgs a = b.args(src.p, n, H, W, nbins);
    a.tcdf = tc.p; a.tcentre = tx.p; a.nt = nt; a.t_stride = n_tables == 1 ? 0 : nt; a.out = dst.p;
    for (int st = 0; st < HIST_STAGES; ++st) HIPCHECK(p3d_hist_launch(st, a, nullptr));
    dst.get(out, (size_t)n * N);
    API_END
}

int p3d_match_hist_maps(int device, const float* maps, const float* targets, int n, int H, int W, int nbins, float* out) {
    API_BEGIN
    hist_shape("match_hist_maps", maps, out, n, H, W, nbins);
    if (!targets) throw P3dError("match_hist_maps: null argument");
    metric_args(device, maps, maps, 1, 1, out);
    const long long N = (long long)H * W;
    DevArr<float> src((size_t)n * N, maps), tgt((size_t)n * N, targets), dst((size_t)n * N);
    HistBufs bt(n, N, nbins), bs(n, N, nbins);
    HistChain c;
    c.has_target = true;
    c.target = bt.args(tgt.p, n, H, W, nbins);
    c.source = bs.args(src.p, n, H, W, nbins);
    c.source.tcdf = bt.cdf.p; c.source.tcentre = bt.centre.p; c.source.nt = nbins; c.source.t_stride = nbins; c.source.out = dst.p;
    HIPCHECK(p3d_hist_chain_launch(c, nullptr));
    dst.get(out, (size_t)n * N);
    API_END
}

}  // extern "C"
namespace {
// ---- fixation priors (include/p3d_hip.h; the handle's part in net_prior.inc, the kernels in prior.hip) -------------------------
// Counts -> float32 -> BLUR -> NORM (max) on stream s: the conversion, then the shared launch sequence on one map, in place on
// `map` [H * W] (device).  Returns the float32 maximum of the blurred counts (0: every count was zero, the map is left unscaled).
float prior_finish_launches(hipStream_t s, const unsigned* count, int H, int W, const Stages& st, float* map) {
    const long long N = (long long)H * W;
    StageScratch scratch;
    unsigned* const counters = carve_scratch(s, 1, [&](Carve& c) { scratch.carve(c, st, 1, N, false); });
    HIPCHECK(p3d_prior_float(count, map, N, s));
    PostJob job;
    job.total = 1; job.h = H; job.w = W; job.H = H; job.W = W; job.f32 = map;
    post_sequence(s, st, scratch, counters, 1, job);
    float mnmx[2] = {0.f, 0.f};
    HIPCHECK(copy_now(mnmx, scratch.post.mnmx, sizeof(mnmx), hipMemcpyDeviceToHost, s));
    return mnmx[1];
}
Stages prior_plan(float sigma, int radius, int H, int W) {
    const p3d_postprocess cfg{sigma, radius, P3D_NORM_MAX};
    Stages st;
    st.post = PostPlan(&cfg);                  // the blur's own refusals
    st.post.fits(H, W);
    return st;
}
void prior_finish(p3d_handle* h, float sigma, int radius, float* out) {
    h->prior_acc.need_open("prior_finish");
    const int H = h->prior_acc.H, W = h->prior_acc.W;
    const Stages plan = prior_plan(sigma, radius, H, W);
    if (h->prior_acc.n_maps < 1) throw P3dError("prior_finish: the accumulator holds no maps");
    if (h->prior_underflowed()) throw P3dError("prior_finish: a subtraction took a count below zero (maps were taken out that were never added); open the accumulator again");
    const hipStream_t s = h->stream;
    DevArr<float> map((size_t)H * W);          // the handle's from prior.take on
    StageTimer tm(true, 2);
    tm.mark(0, s);
    const float mx = prior_finish_launches(s, h->prior_acc.count, H, W, plan, map.p);
    tm.mark(1, s);
    HIPCHECK(hipStreamSynchronize(s));
    if (!(mx > 0.f)) throw P3dError("prior_finish: every count is zero");
    h->prior.ms[1] = tm.ms(0);
    if (out) HIPCHECK(copy_now(out, map.p, (size_t)H * W * sizeof(float), hipMemcpyDeviceToHost, s));
    h->prior.take(std::move(map), H, W);
}
}  // namespace
extern "C" {

int p3d_prior_open(p3d_handle* h, int H, int W, int kind) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->prior_open(H, W, kind);
    API_END
}

int p3d_prior_close(p3d_handle* h) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->prior_acc = p3d_handle::PriorAcc();
    API_END
}

int p3d_prior_info(p3d_handle* h, int* H, int* W, int* kind, int64_t* n_maps) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    h->prior_acc.need_open("prior_info");
    if (H) *H = h->prior_acc.H;
    if (W) *W = h->prior_acc.W;
    if (kind) *kind = h->prior_acc.kind;
    if (n_maps) *n_maps = h->prior_acc.n_maps;
    API_END
}

int p3d_prior_add(p3d_handle* h, const unsigned char* maps, int64_t n, int sign) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->prior_add(maps, n, sign);
    API_END
}

int p3d_prior_counts(p3d_handle* h, uint32_t* out, int64_t* n_maps) {
    API_BEGIN
    if (!h || !out) throw P3dError("null argument");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->prior_acc.need_open("prior_counts");
    if (h->prior_underflowed()) throw P3dError("prior_counts: a subtraction took a count below zero (maps were taken out that were never added); open the accumulator again");
    HIPCHECK(copy_now(out, h->prior_acc.count, (size_t)h->prior_acc.H * h->prior_acc.W * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    if (n_maps) *n_maps = h->prior_acc.n_maps;
    API_END
}

int p3d_prior_finish(p3d_handle* h, float sigma, int radius, float* out) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    HIPCHECK(hipSetDevice(h->cfg.device));
    prior_finish(h, sigma, radius, out);
    API_END
}

int p3d_prior_last_ms(p3d_handle* h, double ms[2]) {
    API_BEGIN
    if (!h || !ms) throw P3dError("null argument");
    ms[0] = h->prior.ms[0]; ms[1] = h->prior.ms[1];
    API_END
}

int p3d_set_prior_map(p3d_handle* h, const float* map, int H, int W) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->set_prior_map(map, H, W);
    API_END
}

int p3d_get_prior_map(p3d_handle* h, float* out, int64_t cap, int* H, int* W) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    if (H) *H = h->prior.H;
    if (W) *W = h->prior.W;
    if (out) {
        if (!h->prior.map) throw P3dError("get_prior_map: the handle has no prior (p3d_prior_finish or p3d_set_prior_map)");
        const int64_t n = (int64_t)h->prior.H * h->prior.W;
        if (cap < n) throw P3dError("get_prior_map: room for " + std::to_string(cap) + " floats, " + std::to_string(n) + " needed");
        HIPCHECK(hipSetDevice(h->cfg.device));
        HIPCHECK(copy_now(out, h->prior.map, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    }
    API_END
}

int p3d_set_prior_stage(p3d_handle* h, int mode, float a) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    h->set_prior_stage(mode, a);
    API_END
}

int p3d_get_prior_stage(p3d_handle* h, int* mode, float* a) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    if (mode) *mode = h->prior.mode;
    if (a) *a = h->prior.a;
    API_END
}

int p3d_set_eval_extra_prior(p3d_handle* h, int flags) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->set_eval_extra_prior(flags);
    API_END
}

int p3d_debug_prior_count(int device, int kind, const unsigned char* maps, int64_t n, int H, int W, int sign, const uint32_t* counts_in,
                          int offset, uint32_t* counts_out, int* flag_out) {
    API_BEGIN
    metric_args(device, maps, maps, 1, 1, counts_out);
    if (!flag_out) throw P3dError("null argument");
    if (H < 1 || W < 1 || (long long)H * W > INT32_MAX / 2) throw P3dError("prior_count: maps are H x W bytes, 1 <= H * W <= 2^30");
    if (n < 1 || n > P3D_PRIOR_MAX_MAPS) throw P3dError("prior_count: 1 .. P3D_PRIOR_MAX_MAPS maps");
    if (kind != P3D_PRIOR_FIXATIONS && kind != P3D_PRIOR_BYTES) throw P3dError("prior_count: unknown kind " + std::to_string(kind));
    if (sign != 1 && sign != -1) throw P3dError("prior_count: sign must be +1 or -1");
    if (offset < 0 || offset > 3) throw P3dError("prior_count: offset in [0, 3]");
    const size_t N = (size_t)H * W;
    Guarded<unsigned char> src((size_t)n * N, 16, (size_t)offset, maps);
    Guarded<uint32_t> cnt(N, 8, 0, counts_in), flag(1, 2, 0, nullptr);
    PriorCountArgs a;
    a.maps = src.data(); a.n = n; a.n_pix = (long long)N; a.kind = kind; a.sign = sign; a.count = cnt.data(); a.flag = flag.data();
    HIPCHECK(p3d_prior_count_launch(a, nullptr));
    uint32_t f = 0;
    cnt.back(counts_out, "prior_count");
    flag.back(&f, "prior_count");
    src.unchanged("prior_count");
    if (f > 1) throw P3dError("prior_count: the flag holds " + std::to_string(f));
    *flag_out = (int)f;
    API_END
}

int p3d_debug_prior_count_plan(int64_t n, int H, int W, int offset, int64_t* words, int64_t* singles, int* slices) {
    API_BEGIN
    if (!words || !singles || !slices) throw P3dError("null argument");
    unsigned dummy[2];
    PriorCountArgs a;
    a.maps = reinterpret_cast<const unsigned char*>((uintptr_t)256 + (uintptr_t)(offset & 3)); a.n = n; a.n_pix = (long long)H * W;
    a.count = dummy; a.flag = dummy + 1;
    if (H < 1 || W < 1 || !p3d_prior_count_plan(a)) throw P3dError("prior_count_plan: arguments the launcher refuses");
    *words = a.words; *singles = a.singles; *slices = a.slices;
    API_END
}

int p3d_debug_prior_apply(int device, int mode, float a, const float* maps, int n, int H, int W, const float* prior, int offset, float* out) {
    API_BEGIN
    metric_args(device, maps, prior, 1, 1, out);
    if (n < 1 || n > 65535 || H < 1 || W < 1 || (long long)H * W > INT32_MAX / 2) throw P3dError("prior_apply: 1 .. 65535 maps of H x W floats, 1 <= H * W <= 2^30");
    p3d_handle::PriorMap::stage_check(mode, a);
    if (mode == P3D_PRIOR_OFF) throw P3dError("prior_apply: the mode is P3D_PRIOR_MUL or P3D_PRIOR_MIX");
    offset_check("prior_apply", offset);
    const size_t N = (size_t)H * W;
    Guarded<float> v((size_t)n * N, 8, (size_t)(offset & 3), maps), g(N, 8, (size_t)((offset >> 2) & 3), prior);
    PriorApplyArgs q;
    q.maps = v.data(); q.prior = g.data(); q.n = n; q.n_pix = (int)N; q.mode = mode; q.nblk = p3d_post_blocks((long long)N);
    q.a = a; q.b = (float)(1.0 - (double)a);
    HIPCHECK(p3d_prior_apply_launch(q, nullptr));
    v.back(out, "prior_apply");
    g.unchanged("prior_apply");
    API_END
}

// ---- fixation pool and shuffled AUC in the evaluation pass (include/p3d_hip.h; the handle's part in net_fixpool.inc, fixpool.hip) ----
int p3d_fixpool_open(p3d_handle* h, int H, int W, int64_t capacity) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->fixpool_open(H, W, capacity);
    API_END
}

int p3d_fixpool_close(p3d_handle* h) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->fixpool = p3d_handle::FixPool();
    API_END
}

int p3d_fixpool_info(p3d_handle* h, int* H, int* W, int64_t* capacity, int64_t* words_per_map, int64_t* n_filled) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    h->fixpool.need_open("fixpool_info");
    if (H) *H = h->fixpool.H;
    if (W) *W = h->fixpool.W;
    if (capacity) *capacity = h->fixpool.cap;
    if (words_per_map) *words_per_map = h->fixpool.nw;
    if (n_filled) *n_filled = (int64_t)std::count(h->fixpool.filled.begin(), h->fixpool.filled.end(), (char)1);
    API_END
}

int p3d_fixpool_put(p3d_handle* h, int64_t first, const unsigned char* maps, int64_t n) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->fixpool_put(first, maps, n);
    API_END
}

int p3d_fixpool_get(p3d_handle* h, int64_t first, int64_t n, uint64_t* words) {
    API_BEGIN
    if (!h || !words) throw P3dError("null argument");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->fixpool.need_open("fixpool_get");
    if (n < 1 || first < 0 || first > h->fixpool.cap - n)
        throw P3dError("fixpool_get: slots " + std::to_string(first) + " .. " + std::to_string(first + n - 1) + " are not inside [0, " + std::to_string(h->fixpool.cap) + ")");
    for (int64_t i = first; i < first + n; ++i)
        if (!h->fixpool.filled[(size_t)i]) throw P3dError("fixpool_get: slot " + std::to_string(i) + " was never filled (p3d_fixpool_put)");
    HIPCHECK(copy_now(words, h->fixpool.words + first * h->fixpool.nw, (size_t)n * h->fixpool.nw * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    API_END
}

int p3d_fixpool_last_ms(p3d_handle* h, double ms[4]) {
    API_BEGIN
    if (!h || !ms) throw P3dError("null argument");
    ms[0] = h->fixpool_ms[0]; ms[1] = h->fixpool_ms[1]; ms[2] = h->fixpool_ms[2]; ms[3] = h->fixpool_ms[3];
    API_END
}

int p3d_eval_shuffled_begin(p3d_handle* h, const int* ids, int M, uint32_t* n_other_out) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->shuffled_begin(ids, h->pred->N, M, n_other_out);
    API_END
}

int p3d_eval_shuffled_draws(p3d_handle* h, const int* ranks, const int* n_rows, int n_rep, double step) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    h->shuffled_draws(ranks, n_rows, n_rep, step);
    API_END
}

int p3d_last_eval_shuffled(p3d_handle* h, double* per_rep, int64_t cap) {
    API_BEGIN
    if (!h || !per_rep) throw P3dError("null argument");
    if (!h->fixpool.have) throw P3dError("last_eval_shuffled: no evaluation has run armed (p3d_eval_shuffled_draws)");
    if (cap < (int64_t)h->fixpool.last.size())
        throw P3dError("last_eval_shuffled: room for " + std::to_string(cap) + " doubles, " + std::to_string(h->fixpool.last.size()) + " needed");
    std::copy(h->fixpool.last.begin(), h->fixpool.last.end(), per_rep);
    API_END
}

}  // extern "C"
namespace {
void fix_shape(const char* what, int H, int W) {
    if (H < 1 || W < 1 || (long long)H * W > INT32_MAX / 2) throw P3dError(std::string(what) + ": maps are H x W bytes, 1 <= H * W <= 2^30");
}
// op level: the union of B rows of M slots of a pool of `cap` packed maps, every device buffer between guard words
struct FixUnionRun {
    long long nw; int nsb, B;
    Guarded<unsigned long long> pool, uni; Guarded<unsigned> prefix, bsum, n_other, counter; Guarded<int> ids;
    FixUnionArgs a;
    FixUnionRun(const uint64_t* words, int cap, int H, int W, const int* idv, int B_, int M)
        : nw(p3d_fix_words((long long)H * W)), nsb(p3d_fix_scan_blocks(nw)), B(B_),
          pool((size_t)cap * nw, 4, 0, reinterpret_cast<const unsigned long long*>(words)), uni((size_t)B_ * nw, 4, 0, nullptr),
          prefix((size_t)B_ * nw, 8, 0, nullptr), bsum((size_t)B_ * nsb, 8, 0, nullptr), n_other((size_t)B_, 8, 0, nullptr),
          counter((size_t)B_, 8, 0, nullptr), ids((size_t)B_ * M, 8, 0, idv) {
        a.pool = pool.data(); a.nw = nw; a.ids = ids.data(); a.B = B; a.M = M; a.nsb = nsb;
        a.uni = uni.data(); a.prefix = prefix.data(); a.bsum = bsum.data(); a.n_other = n_other.data(); a.counter = counter.data();
        HIPCHECK(p3d_fix_union_launch(a, nullptr));
    }
    // uni [B][nw], the exclusive prefix over the whole map [B][nw] (block sum + block-local prefix), n_other [B]; guards intact
    void back(uint64_t* uni_out, uint32_t* prefix_out, uint32_t* n_other_out, const char* what) {
        std::vector<unsigned> local((size_t)B * nw), bs((size_t)B * nsb), zero((size_t)B, 1u);
        uni.back(reinterpret_cast<unsigned long long*>(uni_out), what);
        prefix.back(local.data(), what);
        bsum.back(bs.data(), what);
        n_other.back(n_other_out, what);
        counter.back(zero.data(), what);
        pool.unchanged(what);
        ids.unchanged(what);
        for (unsigned z : zero) if (z != 0u) throw P3dError(std::string(what) + ": an arrival counter was left at " + std::to_string(z));
        if (prefix_out)
            for (int b = 0; b < B; ++b)
                for (long long k = 0; k < nw; ++k) prefix_out[(size_t)b * nw + k] = bs[(size_t)b * nsb + k / P3D_FIX_SCAN_WORDS] + local[(size_t)b * nw + k];
    }
};
void fix_ids_check(const char* what, const int* ids, int cap, int B, int M) {
    if (!ids) throw P3dError("null argument");
    if (cap < 1 || B < 1 || B > 65535) throw P3dError(std::string(what) + ": 1 .. 65535 rows over a pool of at least one map");
    if (M < 1 || M > 64) throw P3dError(std::string(what) + ": 1 .. 64 other maps per clip, not " + std::to_string(M));
    for (size_t i = 0; i < (size_t)B * M; ++i)
        if (ids[i] < 0 || ids[i] >= cap) throw P3dError(std::string(what) + ": slot " + std::to_string(ids[i]) + " is outside [0, " + std::to_string(cap) + ")");
}
}  // namespace
extern "C" {

int p3d_debug_fix_pack(int device, const unsigned char* maps, int n, int H, int W, int offset, uint64_t* words) {
    API_BEGIN
    metric_args(device, maps, maps, 1, 1, words);
    fix_shape("fix_pack", H, W);
    if (n < 1 || n > 65535) throw P3dError("fix_pack: 1 .. 65535 maps");
    if (offset < 0 || offset > 3) throw P3dError("fix_pack: offset in [0, 3]");
    const size_t N = (size_t)H * W, nw = (size_t)p3d_fix_words((long long)N);
    Guarded<unsigned char> src((size_t)n * N, 16, (size_t)offset, maps);
    Guarded<unsigned long long> dst((size_t)n * nw, 4, 0, nullptr);
    FixPackArgs a;
    a.maps = src.data(); a.n = n; a.n_pix = (long long)N; a.words = dst.data();
    HIPCHECK(p3d_fix_pack_launch(a, nullptr));
    dst.back(reinterpret_cast<unsigned long long*>(words), "fix_pack");
    src.unchanged("fix_pack");
    API_END
}

int p3d_debug_fix_union(int device, const uint64_t* pool, int capacity, int H, int W, const int* ids, int B, int M, uint64_t* uni,
                        uint32_t* prefix, uint32_t* n_other) {
    API_BEGIN
    metric_args(device, pool, pool, 1, 1, uni);
    if (!n_other) throw P3dError("null argument");
    fix_shape("fix_union", H, W);
    fix_ids_check("fix_union", ids, capacity, B, M);
    FixUnionRun u(pool, capacity, H, W, ids, B, M);
    u.back(uni, prefix, n_other, "fix_union");
    API_END
}

int p3d_debug_fix_select(int device, const uint64_t* pool, int capacity, int H, int W, const int* ids, int B, int M, const int* ranks,
                         const int* n_rows, int n_rep, int* out) {
    API_BEGIN
    metric_args(device, pool, pool, 1, 1, out);
    fix_shape("fix_select", H, W);
    fix_ids_check("fix_select", ids, capacity, B, M);
    FixUnionRun u(pool, capacity, H, W, ids, B, M);
    std::vector<uint32_t> n_other((size_t)B);
    std::vector<uint64_t> uni((size_t)B * u.nw);
    u.back(uni.data(), nullptr, n_other.data(), "fix_select");
    p3d_handle::FixPool::check_draws("fix_select", ranks, n_rows, n_other.data(), B, n_rep, 1.0);
    std::vector<int> meta((size_t)B * 3, 0);
    long long at = 0;
    int max_rows = 0;
    for (int b = 0; b < B; ++b) { meta[b * 3 + 2] = (int)at; at += (long long)n_rows[b] * n_rep; max_rows = std::max(max_rows, n_rows[b]); }
    if (at < 1) throw P3dError("fix_select: no rank to select");
    Guarded<int> dranks((size_t)at, 8, 0, ranks), dout((size_t)at, 8, 0, nullptr), dmeta(meta.size(), 8, 0, meta.data()), drows((size_t)B, 8, 0, n_rows);
    FixSelectArgs q;
    q.uni = u.a.uni; q.prefix = u.a.prefix; q.bsum = u.a.bsum; q.n_other = u.a.n_other; q.nw = u.nw; q.B = B; q.nsb = u.nsb; q.n_rep = n_rep;
    q.max_rows = max_rows; q.meta = dmeta.data(); q.n_rows = drows.data(); q.ranks = dranks.data(); q.out = dout.data();
    HIPCHECK(p3d_fix_select_launch(q, nullptr));
    dout.back(out, "fix_select");
    dranks.unchanged("fix_select"); dmeta.unchanged("fix_select"); drows.unchanged("fix_select");
    std::vector<uint64_t> uni2(uni.size());
    std::vector<uint32_t> n2((size_t)B);
    u.back(uni2.data(), nullptr, n2.data(), "fix_select");      // the select reads the union: same words, guards intact
    if (uni2 != uni || n2 != n_other) throw P3dError("fix_select: a launch wrote to a read-only buffer");
    API_END
}

// ---- the evaluation hooks: p3d_debug_eval_maps and its five supersets, one body ---------------------------------------------------
}  // extern "C"
namespace {
// Everything the richest hook, p3d_debug_eval_maps_shuffled, takes; a hook that lacks an argument leaves it off / null.  The hooks
// differ in two more ways than in what they pass, and each is a field: prior_as_baseline and shuffled.
struct EvalHook {
    int device; const float* maps; int n_maps, h, w, elem_stride; EvalInputs in;
    const p3d_postprocess* cfg = nullptr; const p3d_hist_match* match = nullptr;
    int flags = 0; const float* baseline = nullptr; double* extra = nullptr;
    const float* prior = nullptr; int mode = P3D_PRIOR_OFF; float a = 0.f;
    // _prior alone: P3D_EVAL_INFO_GAIN with a null baseline is not refused but scores over the prior, copied device to device (and
    // the prior is then checked whatever the mode); every other hook leaves that case to eval_extra_check, which refuses it
    bool prior_as_baseline = false;
    // _shuffled alone: the pool is packed, the union taken and the armed sequence runs; the ten arguments below are its own
    bool shuffled = false;
    const unsigned char* pool_maps = nullptr; int capacity = 0; const int* ids = nullptr; int M = 0; const int* ranks = nullptr;
    const int* n_rows = nullptr; int sh_n_rep = 0; double sh_step = 0.0; uint32_t* n_other = nullptr; double* per_rep = nullptr;
};
void eval_hook(const EvalHook& q) {
    const EvalInputs& in = q.in;
    const int H = in.H, W = in.W, n_maps = q.n_maps;
    EvalRequest rq;
    Stages& st = rq.stages;
    st = Stages(nullptr, q.match, nullptr, q.mode, q.a, H, W);      // match_parse: ahead of any device call
    metric_args(q.device, q.maps, q.maps, n_maps, 1, in.out);
    if (q.h < 1 || q.w < 1 || q.elem_stride < 1) throw P3dError("eval: empty map");
    if (q.flags && !q.extra) throw P3dError("null argument");
    if (q.shuffled) {
        if (!q.pool_maps || !q.n_other || !q.per_rep) throw P3dError("null argument");
        fix_shape("eval_shuffled", H, W);
        if (q.capacity < 1 || q.capacity > 65535) throw P3dError("eval_shuffled: 1 .. 65535 pool maps");
        fix_ids_check("eval_shuffled", q.ids, q.capacity, n_maps, q.M);
    }
    p3d_handle::PriorMap::stage_check(q.mode, q.a);
    const bool from_prior = q.prior_as_baseline && (q.flags & P3D_EVAL_INFO_GAIN) && !q.baseline;
    if (q.mode != P3D_PRIOR_OFF || from_prior || q.prior) p3d_handle::PriorMap::check(q.prior, H, W);
    if (!from_prior) p3d_handle::Extra::check(q.flags, q.baseline, H, W);           // (the baseline of the hook has the evaluation's size)
    else if (q.flags & ~(P3D_EVAL_KLDIV | P3D_EVAL_INFO_GAIN)) throw P3dError("eval_extra: unknown flags " + std::to_string(q.flags));
    const long long per_map = (long long)q.h * q.w * q.elem_stride;
    const bool ig = (q.flags & P3D_EVAL_INFO_GAIN) != 0;
    DevArr<float> src((size_t)n_maps * per_map, q.maps), base(ig ? (size_t)H * W : 1), dprior(q.prior ? (size_t)H * W : 1, q.prior);
    DevArr<double> bstat(3);
    if (ig) p3d_handle::Extra::upload(from_prior ? dprior.p : q.baseline, H, W, base.p, bstat.p, nullptr,
                                          from_prior ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
    const EvalExtra x{q.flags, ig ? base.p : nullptr, ig ? bstat.p : nullptr, H, W, q.extra};
    st.prior.map = dprior.p;
    // the pool packed here, then the union: the launches the handle issues, on private buffers
    std::unique_ptr<FixUnionRun> u;
    ShuffledEval sh{};
    if (q.shuffled) {
        const size_t N = (size_t)H * W, nw = (size_t)p3d_fix_words((long long)N);
        DevArr<unsigned char> pm((size_t)q.capacity * N, q.pool_maps);
        DevArr<unsigned long long> words((size_t)q.capacity * nw);
        FixPackArgs pk;
        pk.maps = pm.p; pk.n = q.capacity; pk.n_pix = (long long)N; pk.words = words.p;
        HIPCHECK(p3d_fix_pack_launch(pk, nullptr));
        std::vector<uint64_t> packed((size_t)q.capacity * nw);
        words.get(reinterpret_cast<unsigned long long*>(packed.data()), packed.size());
        u.reset(new FixUnionRun(packed.data(), q.capacity, H, W, q.ids, n_maps, q.M));
        std::vector<uint64_t> uni((size_t)n_maps * nw);
        u->back(uni.data(), nullptr, q.n_other, "eval_shuffled");
        sh = ShuffledEval{u->a.uni, u->a.prefix, u->a.bsum, u->a.n_other, q.n_other, (long long)nw, H, W, q.ranks, q.n_rows, q.sh_n_rep, q.sh_step,
                          q.per_rep, nullptr};
    }
    st.post = PostPlan(q.cfg);                 // its refusals come last, as they did when eval_maps parsed the setting
    rq.src = {src.p, per_map, q.elem_stride, n_maps, q.h, q.w};
    rq.in = in;
    rq.extra = &x;
    rq.sh = q.shuffled ? &sh : nullptr;
    eval_maps(nullptr, rq);
}
}  // namespace
extern "C" {

int p3d_debug_eval_maps(int device, const float* maps, int n_maps, int h, int w, int elem_stride, const unsigned char* density,
                        int Hd, int Wd, const unsigned char* fixation, int H, int W, const double* jitter, const int* borji_idx,
                        const int* n_fix, int n_rep, double step_size, double* out) {
    API_BEGIN
    eval_hook({device, maps, n_maps, h, w, elem_stride, {density, Hd, Wd, fixation, H, W, jitter, borji_idx, n_fix, n_rep, step_size, out}});
    API_END
}

int p3d_debug_eval_maps_post(int device, const float* maps, int n_maps, int h, int w, int elem_stride, const unsigned char* density,
                             int Hd, int Wd, const unsigned char* fixation, int H, int W, const double* jitter, const int* borji_idx,
                             const int* n_fix, int n_rep, double step_size, double* out, const p3d_postprocess* cfg) {
    API_BEGIN
    EvalHook q{device, maps, n_maps, h, w, elem_stride, {density, Hd, Wd, fixation, H, W, jitter, borji_idx, n_fix, n_rep, step_size, out}};
    q.cfg = cfg;
    eval_hook(q);
    API_END
}

int p3d_debug_eval_maps_match(int device, const float* maps, int n_maps, int h, int w, int elem_stride, const unsigned char* density,
                              int Hd, int Wd, const unsigned char* fixation, int H, int W, const double* jitter, const int* borji_idx,
                              const int* n_fix, int n_rep, double step_size, double* out, const p3d_postprocess* cfg,
                              const p3d_hist_match* match) {
    API_BEGIN
    EvalHook q{device, maps, n_maps, h, w, elem_stride, {density, Hd, Wd, fixation, H, W, jitter, borji_idx, n_fix, n_rep, step_size, out}};
    q.cfg = cfg; q.match = match;
    eval_hook(q);
    API_END
}

int p3d_debug_eval_maps_extra(int device, const float* maps, int n_maps, int h, int w, int elem_stride, const unsigned char* density,
                              int Hd, int Wd, const unsigned char* fixation, int H, int W, const double* jitter, const int* borji_idx,
                              const int* n_fix, int n_rep, double step_size, double* out, const p3d_postprocess* cfg,
                              const p3d_hist_match* match, int flags, const float* baseline, double* extra) {
    API_BEGIN
    EvalHook q{device, maps, n_maps, h, w, elem_stride, {density, Hd, Wd, fixation, H, W, jitter, borji_idx, n_fix, n_rep, step_size, out}};
    q.cfg = cfg; q.match = match; q.flags = flags; q.baseline = baseline; q.extra = extra;
    eval_hook(q);
    API_END
}

int p3d_debug_eval_maps_prior(int device, const float* maps, int n_maps, int h, int w, int elem_stride, const unsigned char* density,
                              int Hd, int Wd, const unsigned char* fixation, int H, int W, const double* jitter, const int* borji_idx,
                              const int* n_fix, int n_rep, double step_size, double* out, const p3d_postprocess* cfg,
                              const p3d_hist_match* match, int flags, const float* baseline, double* extra, const float* prior, int mode,
                              float a) {
    API_BEGIN
    EvalHook q{device, maps, n_maps, h, w, elem_stride, {density, Hd, Wd, fixation, H, W, jitter, borji_idx, n_fix, n_rep, step_size, out}};
    q.cfg = cfg; q.match = match; q.flags = flags; q.baseline = baseline; q.extra = extra; q.prior = prior; q.mode = mode; q.a = a;
    q.prior_as_baseline = true;
    eval_hook(q);
    API_END
}

int p3d_debug_eval_maps_shuffled(int device, const float* maps, int n_maps, int h, int w, int elem_stride, const unsigned char* density,
                                 int Hd, int Wd, const unsigned char* fixation, int H, int W, const double* jitter, const int* borji_idx,
                                 const int* n_fix, int n_rep, double step_size, double* out, const p3d_postprocess* cfg,
                                 const p3d_hist_match* match, int flags, const float* baseline, double* extra, const float* prior, int mode,
                                 float a, const unsigned char* pool_maps, int capacity, const int* ids, int M, const int* ranks,
                                 const int* n_rows, int sh_n_rep, double sh_step, uint32_t* n_other, double* per_rep) {
    API_BEGIN
    EvalHook q{device, maps, n_maps, h, w, elem_stride, {density, Hd, Wd, fixation, H, W, jitter, borji_idx, n_fix, n_rep, step_size, out}};
    q.cfg = cfg; q.match = match; q.flags = flags; q.baseline = baseline; q.extra = extra; q.prior = prior; q.mode = mode; q.a = a;
    q.shuffled = true;
    q.pool_maps = pool_maps; q.capacity = capacity; q.ids = ids; q.M = M; q.ranks = ranks; q.n_rows = n_rows; q.sh_n_rep = sh_n_rep;
    q.sh_step = sh_step; q.n_other = n_other; q.per_rep = per_rep;
    eval_hook(q);
    API_END
}

// ---- resident video inference (include/p3d_hip.h; the handle's part in net_video.inc, the kernels in video.hip) --------------
int p3d_video_open(p3d_handle* h, int frames, int mode) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->video_open(frames, mode);
    API_END
}

int p3d_video_close(p3d_handle* h) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->video_close();
    API_END
}

int p3d_video_info(p3d_handle* h, int* frames, int* mode, int* last_start) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    h->video.need_open("video_info");
    if (frames) *frames = h->video.F;
    if (mode) *mode = h->video.mode;
    if (last_start) *last_start = h->video.last;
    API_END
}

int p3d_video_put_frames(p3d_handle* h, int first, const float* x, int n) {
    API_BEGIN
    if (!h || !x) throw P3dError("null argument");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->video_put_frames(first, x, n);
    API_END
}

int p3d_video_put_frames_u8(p3d_handle* h, int first, const unsigned char* bgr, int n, int H0, int W0, const float mean_rgb[3]) {
    API_BEGIN
    if (!h || !bgr || !mean_rgb) throw P3dError("null argument");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->video_put_frames_u8(first, bgr, n, H0, W0, mean_rgb);
    API_END
}

int p3d_video_predict(p3d_handle* h, const int* starts, int n_windows) {
    API_BEGIN
    if (!h || !starts) throw P3dError("null argument");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->video_predict(starts, n_windows);
    API_END
}

int p3d_video_predict_shots(p3d_handle* h, const int* starts, int n_windows) {
    API_BEGIN
    if (!h || !starts) throw P3dError("null argument");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->video_predict_shots(starts, n_windows);
    API_END
}

int p3d_video_last_ms(p3d_handle* h, double ms[2]) {
    API_BEGIN
    if (!h || !ms) throw P3dError("null argument");
    if (!h->video.is_open || !h->video.timed) throw P3dError("video_last_ms: no p3d_video_predict has run on the open video");
    HIPCHECK(hipSetDevice(h->cfg.device));
    float g = 0.f, sc = 0.f;
    HIPCHECK(hipEventElapsedTime(&g, h->video.ev[0], h->video.ev[1]));
    HIPCHECK(hipEventElapsedTime(&sc, h->video.ev[2], h->video.ev[3]));
    ms[0] = (double)g; ms[1] = (double)sc;
    API_END
}

}  // extern "C"
namespace {
// Frames first .. first + n - 1 of the open video as a read-out's source.  Refused here, in this order and before any scratch is
// asked for (a refusal changes nothing): no open video, the range, more than `most` frames, what p3d_set_video_temporal's filter
// needs and, where `predicted` is asked for, a frame without a prediction.
struct VideoSource {
    p3d_handle* h; const char* who; int first, n; bool temporal;
    VideoSource(p3d_handle* h_, const char* who_, int first_, int n_, bool predicted = true, int most = INT32_MAX)
        : h(h_), who(who_), first(first_), n(n_), temporal(h_->temporal.cfg.on()) {
        h->video.need_open(who);
        h->video.range(who, first, n);
        if (n > most) throw P3dError(std::string(who) + ": 1 .. " + std::to_string(most) + " maps");
        if (temporal) h->video_temporal_check(who, first, n);
        if (predicted) h->video.need_predicted(who, first, n);
    }
    // floats of scratch the maps need: the filtered maps under either mode, the divided sums under MEAN
    size_t extra() const {
        return temporal || h->video.mode == VIDEO_MEAN ? (size_t)n * (size_t)h->vid_hw() + (temporal ? h->video_temporal_table(n) : 0) : 0;
    }
    // queues whatever makes the maps readable; -> the maps [n][hw]
    const float* queue(hipStream_t s, float* scratch) const {
        return temporal ? h->video_temporal(who, first, n, scratch, s) : h->video_finalize(who, first, n, scratch, s);
    }
    void operator()(hipStream_t s, float* scratch, std::vector<PostRun>& runs) const { runs.push_back({queue(s, scratch), h->vid_hw(), 1, n}); }
};
}  // namespace
extern "C" {

int p3d_video_get_maps(p3d_handle* h, int first, int n, float* maps, int32_t* counts) {
    API_BEGIN
    if (!h || !maps) throw P3dError("null argument");
    HIPCHECK(hipSetDevice(h->cfg.device));
    const VideoSource src(h, "video_get_maps", first, n, false);      // (a frame without a prediction: refused by video_finalize)
    const hipStream_t s = h->stream;
    float* slab = nullptr;
    unsigned* counters = nullptr;
    if (src.extra()) HIPCHECK(p3d_stream_scratch(s, src.extra(), 0, &slab, &counters));
    HIPCHECK(copy_now(maps, src.queue(s, slab), (size_t)n * (size_t)h->vid_hw() * 4, hipMemcpyDeviceToHost, s));
    if (counts) memcpy(counts, h->video.count.data() + first, (size_t)n * sizeof(int32_t));
    API_END
}

int p3d_video_maps_u8(p3d_handle* h, int first, int n, float scale, int H, int W, unsigned char* out, double* stage_ms) {
    API_BEGIN
    if (!h || !out) throw P3dError("null argument");
    if (H < 1 || W < 1) throw P3dError("video_maps_u8: empty map");
    if ((long long)H * W > INT32_MAX) throw P3dError("video_maps_u8: H * W exceeds the kernel's int32 in-map offsets");
    HIPCHECK(hipSetDevice(h->cfg.device));
    const VideoSource src(h, "video_maps_u8", first, n);
    if (stage_ms) stage_ms[0] = stage_ms[1] = 0.0;
    maps_u8_chain(h, n, h->pred->H, h->pred->W, scale, H, W, out, stage_ms, src.extra(), src);
    API_END
}

}  // extern "C"
namespace {
// ---- what every stage's entry points share ----------------------------------------------------------------------------------------
// The shape every read-out of 8-bit maps takes; bound: what H * W exceeds, in the refusal's words
void map_shape_check(const char* who, int n, int H, int W, long long max_pixels, const char* bound) {
    if (n < 1 || n > 65535) throw P3dError(std::string(who) + ": 1 .. 65535 maps");
    if (H < 1 || W < 1) throw P3dError(std::string(who) + ": empty map");
    if ((long long)H * W > max_pixels) throw P3dError(std::string(who) + ": H * W exceeds " + bound);
}
// The block sizes of the stages that work on a grid of blocks (qpmap, prefilter, distortion)
bool block_size_ok(int block) { return block == 8 || block == 16 || block == 32 || block == 64 || block == 128; }
void shots_table_check(const char* who, const int32_t* starts, int n_shots, int F);      // (net_shots.inc)
// The open video's installed shot table cut to frames first .. first + n - 1, in frames of the call: its shots cut a stage's filters
// and links.  Empty: no table is installed.
std::vector<int32_t> video_shots_within(const p3d_handle* h, int first, int n) {
    std::vector<int32_t> shots;
    if (h->video.shots.empty()) return shots;
    shots.push_back(0);
    for (int32_t st : h->video.shots)
        if (st > first && st < first + n) shots.push_back(st - first);
    return shots;
}
// ... cut into a video entry's request; shots keeps what the request then names
template <typename Request>
void video_shots_into(const p3d_handle* h, int first, std::vector<int32_t>& shots, Request& r) {
    shots = video_shots_within(h, first, r.n);
    if (!shots.empty()) { r.starts = shots.data(); r.n_shots = (int)shots.size(); }
}
// What a hook sees of its block once a guarded run has passed the guards: the block as it was after the uploads and as it is after
// the copies back.  A buffer is named by the device pointer its take returned.
struct GuardedRun {
    const char* who; const GuardExtents& g; const char* base; const unsigned char* before; const unsigned char* after;
    const unsigned* counters; size_t n_counters;
    const GuardExtents::Extent& extent(const void* dev) const { return g.find((size_t)((const char*)dev - base)); }
    // the buffer as the launches left it, into out
    void read(const void* dev, void* out) const { const GuardExtents::Extent& e = extent(dev); memcpy(out, after + e.at, e.bytes); }
    // a buffer that launches may write, which these launches had no business writing
    void unchanged(const void* dev) const { g.unchanged(who, extent(dev), before, after); }
    void counters_at_zero() const {
        std::vector<unsigned> c(n_counters);
        read(counters, c.data());
        for (unsigned z : c) if (z != 0u) throw P3dError(std::string(who) + ": an arrival counter was left at " + std::to_string(z));
    }
};
// op level: the stage behind the host's bytes.  Ends synchronised.  offset < 0: on the null stream's scratch, as the product lays
// it out.  offset in [0, 15], a hook: the same carve inside one block of the hook's own, the bytes (read-only, `offset` past their
// boundary) and the arrival counters with it, every buffer between guards; a launch that wrote outside its buffer or to an input is
// an error, and `inspect` (or none) then looks at what the launches left.
void stage_on_host_bytes(ByteStage& stage, const unsigned char* sal, int offset = -1,
                         const std::function<void(const GuardedRun&)>& inspect = nullptr) {
    if (offset < 0) {
        DevArr<unsigned char> ds(stage.bytes, sal);
        unsigned* const counters = carve_scratch(nullptr, stage.counters(), [&](Carve& c) { stage.carve(c); });
        stage.upload(nullptr);
        stage.launch(nullptr, ds.p, counters);
        stage.results(nullptr);
        HIPCHECK(hipDeviceSynchronize());
        return;
    }
    const unsigned char* ds = nullptr;
    unsigned* counters = nullptr;
    const auto layout = [&](Carve& c) {
        ds = c.input<unsigned char>(stage.bytes, 1);
        counters = c.take<unsigned>(stage.counters());
        stage.carve(c);
    };
    GuardExtents sized(offset), placed(offset);
    Carve c;
    c.guards = &sized;
    layout(c);
    std::vector<unsigned char> before = sized.image(), after(sized.total);
    memcpy(before.data() + sized.ext[0].at, sal, stage.bytes);
    DevArr<unsigned char> block(sized.total, before.data());
    c = Carve{(char*)block.p, 0, &placed};
    layout(c);
    if (placed.total != sized.total || !(placed.ext == sized.ext)) throw P3dError(std::string(stage.who) + ": the two passes of the carve disagree");
    stage.upload(nullptr);
    block.get(before.data(), sized.total);
    stage.launch(nullptr, ds, counters);
    stage.results(nullptr);
    block.get(after.data(), sized.total);
    sized.verify(stage.who, before.data(), after.data());
    if (inspect) inspect(GuardedRun{stage.who, sized, (const char*)block.p, before.data(), after.data(), counters, stage.counters()});
}
// Frames first .. first + n - 1 of the source the open video keeps, for a call that `verb` ("renders", "reframes") H x W frames
const unsigned char* kept_source(const p3d_handle* h, const char* who, int first, int n, int H, int W, const char* verb) {
    if (H != h->video.H0 || W != h->video.W0)
        throw P3dError(std::string(who) + ": the kept source is " + std::to_string(h->video.H0) + " x " + std::to_string(h->video.W0) + ", the call " + verb + " " +
                       std::to_string(H) + " x " + std::to_string(W));
    for (int f = first; f < first + n; ++f)
        if (!h->video.has_src[(size_t)f]) throw P3dError(std::string(who) + ": frame " + std::to_string(f) + " has no source (it was not put with p3d_video_put_frames_u8)");
    return h->video.source + (size_t)first * (size_t)H * (size_t)W * 3;
}
void need_kept_source(const p3d_handle* h, const char* who) {
    if (!h->video.source) throw P3dError(std::string(who) + ": no frames are given and the video keeps no source (p3d_video_keep_source before the first p3d_video_put_frames_u8)");
}
// A video entry behind the checks of its arguments: at most 65535 of the video's frames through the maps' chain, a Stage built from
// r behind their bytes.  The source comes first, then `ready` (the kept source and the installed shot table into r), then the
// stage, so that what the kept source or the stage refuses is refused after the source's.  stage_ms (null, or n_ms >= 3 values):
// zeroed, then the stage's ms.  (video_score_run, which reads its stage after the chain, issues the same steps itself.)
template <typename Stage, typename Request, typename Ready>
void video_stage_run(p3d_handle* h, Request& r, int first, float scale, unsigned char* maps_out, double* stage_ms, int n_ms, Ready ready) {
    HIPCHECK(hipSetDevice(h->cfg.device));
    const VideoSource src(h, r.who, first, r.n, true, 65535);
    ready();
    r.timed = stage_ms != nullptr;
    Stage stage(r);
    for (int i = 0; stage_ms && i < n_ms; ++i) stage_ms[i] = 0.0;
    maps_u8_chain(h, r.n, h->pred->H, h->pred->W, scale, r.H, r.W, maps_out, nullptr, src.extra(), src, &stage);
    for (int i = 0; stage_ms && i < 3; ++i) stage_ms[i] = stage.ms[i];
}
// ---- scoring 8-bit maps (score_u8.hip; the law in include/p3d_hip.h): one check, one launch sequence and one stage (the
// table of buffer sizes is its own) for p3d_score_maps_u8, the video entries and p3d_debug_score_u8 ----------------------------------
// What one scoring of n maps of H x W bytes asks for; every pointer is host memory.  Whatever is not asked for is not issued.
struct ScoreRequest {
    const char* who; int n, H, W;
    int flags = 0, ties = P3D_SCORE_TIES_REFERENCE;      // the columns -> out [n][5]; 0: none, and the density is not read
    const unsigned char* density = nullptr; const unsigned char* fixation = nullptr; double* out = nullptr;
    // AUC-Borji -> borji [n][n_rep] (null: not asked for): map b's idx_rows[b] x n_rep indices (null: its fixated pixels, counted here)
    const int* idx = nullptr; const int* idx_rows = nullptr; double* borji = nullptr;
    // shuffled AUC -> shuffled [n][n_rep] (null: not asked for): ranks of n_rows[b] x n_rep draws into the union that `pool` holds
    const int* ranks = nullptr; const int* n_rows = nullptr; const p3d_handle* pool = nullptr; double* shuffled = nullptr;
    int n_rep = 0; double step = 0.0;
    // rows_checked, for p3d_score_sweep_u8 and its hook alone: launch waits for the sweeps' preparation, reads the device's counts
    // back and refuses idx_rows above them before it queues the sweeps.  A video caller must never set it: the wait would sit in
    // the middle of its chain, and its rows come from the host's own counts.  top, the test hook alone: the sweep's capture
    // [n][n_rep], carved, bound and copied back when set
    bool rows_checked = false; int* top = nullptr;
    bool timed = false;                                   // events around the stage's moments (ms) and around the sweeps (sweep_ms)
};
// The launches of score_u8.hip and score_auc_u8.hip behind some device bytes: the launch arguments, the tables of the host and the
// device buffers, carved from a caller's scratch.  The constructor refuses what the request's arrays get wrong and queues nothing.
struct ScoreStage : ByteStage {
    const ScoreRequest r;
    ScoreArgs a; ScoreSweepArgs q;
    std::vector<int> nf, meta3, info; std::vector<long long> metaB, metaS;
    size_t totB = 0, totS = 0; int max_rows = 0;
    unsigned char* dd = nullptr; unsigned char* dx = nullptr;
    int* didx = nullptr; int* dtop = nullptr; int* dranks = nullptr; int* dsel = nullptr; int* dmeta3 = nullptr; int* drows = nullptr;
    long long* dmetaB = nullptr; long long* dmetaS = nullptr; double* perB = nullptr; double* perS = nullptr;
    StageTimer sweeps;
    explicit ScoreStage(const ScoreRequest& r);
    bool sweep() const { return r.borji || r.shuffled; }
    size_t counters() const override;
    void carve(Carve& c) override;
    void upload(hipStream_t s) override;
    // pass A and the columns, then the sweeps' preparation (q.info: the device's counts); sweep_rest: the sweeps themselves
    void prepare(hipStream_t s, const unsigned char* sal, unsigned* counters);
    void sweep_rest(hipStream_t s);
    void launch(hipStream_t s, const unsigned char* sal, unsigned* counters) override;
    void results(hipStream_t s) override;
    void check_counts() const;                            // after the results have arrived: the device's counts against nf
    double sweep_ms() const { return sweeps.ev[0] ? (double)sweeps.ms(0) : 0.0; }
};
void score_check(const char* who, const void* density, const void* fixation, int n, int H, int W, int flags, int ties, const void* out) {
    if (!density || !out) throw P3dError("null argument");
    map_shape_check(who, n, H, W, P3D_SCORE_MAX_PIXELS, "2^23, the bound of the 64-bit integer sums");
    if (flags <= 0 || (flags & ~P3D_SCORE_ALL)) throw P3dError(std::string(who) + ": flags are a non-empty set of P3D_SCORE_CC | SIM | JUDD | KL | NSS");
    if (ties != P3D_SCORE_TIES_REFERENCE && ties != P3D_SCORE_TIES_EXPECTED) throw P3dError(std::string(who) + ": ties is P3D_SCORE_TIES_REFERENCE or P3D_SCORE_TIES_EXPECTED");
    if (!fixation && (flags & (P3D_SCORE_JUDD | P3D_SCORE_NSS))) throw P3dError(std::string(who) + ": AUC_Judd and NSS need the fixation maps");
}
ScoreArgs score_args(int n, long long n_pix, int flags, int ties) {
    ScoreArgs a;
    const ScorePlan p = p3d_score_plan(n_pix);
    a.n = n; a.n_pix = (int)n_pix; a.flags = flags; a.ties = ties; a.nblk = p.nblk; a.chunk = p.chunk;
    return a;
}
// Elements of the buffers of one scoring
struct ScoreSizes {
    size_t tab, lut, part, out, counters;
    explicit ScoreSizes(const ScoreArgs& a)
        : tab((size_t)a.n * P3D_SCORE_TAB_WORDS), lut((size_t)a.n * 1024), part((size_t)a.n * a.nblk * 2), out((size_t)a.n * 5), counters((size_t)a.n * 2) {}
};
void score_sequence(const ScoreArgs& a, hipStream_t s) {
    for (int st = 0; st < SCORE_STAGES; ++st) HIPCHECK(p3d_score_launch(st, a, s));
}
}  // namespace
extern "C" {

int p3d_score_maps_u8(int device, const unsigned char* sal, const unsigned char* density, const unsigned char* fixation, int n, int H, int W,
                      int flags, int ties, double* out) {
    API_BEGIN
    if (!sal) throw P3dError("null argument");
    score_check("score_maps_u8", density, fixation, n, H, W, flags, ties, out);
    metric_args(device, sal, density, 1, 1, out);
    ScoreRequest r{"score_maps_u8", n, H, W};
    r.flags = flags; r.ties = ties; r.density = density; r.fixation = fixation; r.out = out;
    ScoreStage stage(r);
    stage_on_host_bytes(stage, sal);
    API_END
}

int p3d_debug_score_u8(int device, const unsigned char* sal, const unsigned char* density, const unsigned char* fixation, int n, int H, int W,
                       int flags, int ties, int offset, uint32_t* hs, uint32_t* hf, uint32_t* hd, uint64_t* sd, double* out) {
    API_BEGIN
    if (!sal) throw P3dError("null argument");
    score_check("debug_score_u8", density, fixation, n, H, W, flags, ties, out);
    offset_check("debug_score_u8", offset);
    metric_args(device, sal, density, 1, 1, out);
    ScoreRequest r{"debug_score_u8", n, H, W};
    r.flags = flags; r.ties = ties; r.density = density; r.fixation = fixation; r.out = out;
    ScoreStage stage(r);
    std::vector<unsigned> t;
    stage_on_host_bytes(stage, sal, offset, [&](const GuardedRun& g) {
        t.resize(g.extent(stage.a.tab).bytes / sizeof(unsigned));
        g.read(stage.a.tab, t.data());
        if (!p3d_score_has(SCORE_TERMS, stage.a)) { g.unchanged(stage.a.lut); g.unchanged(stage.a.part); }      // no pass B: nothing of its was written
        g.counters_at_zero();
    });
    for (int m = 0; m < n; ++m) {
        const unsigned* row = t.data() + (size_t)m * P3D_SCORE_TAB_WORDS;
        if (hs) std::copy(row, row + 256, hs + (size_t)m * 256);
        if (hf) std::copy(row + 256, row + 512, hf + (size_t)m * 256);
        if (hd) std::copy(row + 512, row + 768, hd + (size_t)m * 256);
        if (sd) sd[m] = (uint64_t)row[768] | ((uint64_t)row[769] << 32);
    }
    API_END
}

int p3d_debug_score_plan(int64_t n_pix, int n, int offset, int* blocks_per_map, int* pixels_per_block, int64_t* products_per_lane) {
    API_BEGIN
    if (!blocks_per_map || !pixels_per_block || !products_per_lane) throw P3dError("null argument");
    if (n_pix < 1 || n_pix > P3D_SCORE_MAX_PIXELS || n < 1 || n > 65535 || offset < 0 || offset > 15)
        throw P3dError("debug_score_plan: 1 <= n_pix <= 2^23, 1 .. 65535 maps, offset in [0, 15]");
    const ScorePlan p = p3d_score_plan(n_pix);
    *blocks_per_map = p.nblk; *pixels_per_block = p.chunk;
    *products_per_lane = p3d_score_lane_products(n_pix, n, (unsigned)guard_shift(1, offset), (unsigned)guard_shift(2, offset), (unsigned)guard_shift(3, offset));
    API_END
}

}  // extern "C"
namespace {
// ---- rendering 8-bit maps over their frames (render.hip; the law in include/p3d_hip.h): one check and one launch
// description for p3d_render_u8, the render stage and p3d_debug_render_u8 ------------------------------------------------
// What one rendering of n maps of H x W bytes asks for: frames on the host (uploaded), or on the device where they are (the kept
// source), or neither (the heat map); out on the host.
struct RenderRequest {
    const char* who; int n, H, W;
    const p3d_render* cfg = nullptr;
    const unsigned char* frames = nullptr; const unsigned char* frames_dev = nullptr; unsigned char* out = nullptr;
    bool timed = false;
};
// The launch of render.hip behind some device bytes.  It has no arrival counters: its blocks share nothing.  render_check has
// passed cfg and the shape before one is built.
struct RenderStage : ByteStage {
    const RenderRequest r;
    RenderArgs a;
    unsigned char* df = nullptr; unsigned char* dout = nullptr; unsigned* dtab = nullptr;
    explicit RenderStage(const RenderRequest& r);
    size_t bgr() const { return bytes * 3; }              // the bytes of n frames, in or out
    void carve(Carve& c) override;
    void upload(hipStream_t s) override;
    void launch(hipStream_t s, const unsigned char* sal, unsigned*) override;
    void results(hipStream_t s) override;
};
void render_check(const char* who, const p3d_render* cfg, int n, int H, int W, const void* out) {
    if (!cfg || !out) throw P3dError("null argument");
    map_shape_check(who, n, H, W, P3D_RENDER_MAX_PIXELS, "2^28, the bound of the int32 offsets inside a map");
    if (cfg->contour_level < 0 || cfg->contour_level > 255) throw P3dError(std::string(who) + ": the contour level is 0 (off) .. 255");
    if (cfg->contour_level > 0 && (cfg->contour_thickness < 1 || cfg->contour_thickness > P3D_RENDER_MAX_THICKNESS))
        throw P3dError(std::string(who) + ": the contour thickness is 1 .. 4");
}
RenderArgs render_args(const p3d_render& cfg, int n, int H, int W) {
    RenderArgs a;
    a.n = n; a.H = H; a.W = W; a.level = cfg.contour_level; a.thick = a.level > 0 ? cfg.contour_thickness : 0;
    for (int k = 0; k < 3; ++k) a.contour_bgr[k] = cfg.contour_bgr[k];
    const RenderPlan p = p3d_render_plan(H, W, a.thick);
    a.rows = p.rows; a.cols = p.cols; a.chunk = p.chunk; a.blocks = p.blocks;
    return a;
}

RenderStage::RenderStage(const RenderRequest& r_) : ByteStage(r_), r(r_), a(render_args(*r_.cfg, r_.n, r_.H, r_.W)) {}
void RenderStage::carve(Carve& c) {
    df = r.frames ? c.input<unsigned char>(bgr(), 3) : nullptr;
    dout = c.take<unsigned char>(bgr(), 5);
    dtab = c.input<unsigned>(256);
}
void RenderStage::upload(hipStream_t s) {
    HIPCHECK(hipMemcpyAsync(dtab, r.cfg->table, 256 * sizeof(unsigned), hipMemcpyHostToDevice, s));
    if (df) HIPCHECK(hipMemcpyAsync(df, r.frames, bgr(), hipMemcpyHostToDevice, s));
}
void RenderStage::launch(hipStream_t s, const unsigned char* sal, unsigned*) {
    a.sal = sal; a.frames = df ? df : r.frames_dev; a.out = dout; a.table = dtab;
    HIPCHECK(p3d_render_launch(a, s));
}
void RenderStage::results(hipStream_t s) {
    HIPCHECK(hipMemcpyAsync(r.out, dout, bgr(), hipMemcpyDeviceToHost, s));
}
// p3d_render_u8 (offset < 0) and p3d_debug_render_u8 (offset in [0, 15]): the stage behind the host's bytes
void render_on_host_bytes(const char* who, int device, const unsigned char* sal, const unsigned char* frames, int n, int H, int W,
                          const p3d_render* cfg, int offset, bool hook, unsigned char* out) {
    if (!sal) throw P3dError("null argument");
    render_check(who, cfg, n, H, W, out);
    if (hook) offset_check(who, offset);
    metric_args(device, sal, cfg, 1, 1, out);
    RenderRequest r{who, n, H, W};
    r.cfg = cfg; r.frames = frames; r.out = out;
    RenderStage stage(r);
    stage_on_host_bytes(stage, sal, hook ? offset : -1);
}
}  // namespace
extern "C" {

int p3d_render_u8(int device, const unsigned char* sal, const unsigned char* frames, int n, int H, int W, const p3d_render* cfg,
                  unsigned char* out) {
    API_BEGIN
    render_on_host_bytes("render_u8", device, sal, frames, n, H, W, cfg, -1, false, out);
    API_END
}

int p3d_debug_render_u8(int device, const unsigned char* sal, const unsigned char* frames, int n, int H, int W, const p3d_render* cfg,
                        int offset, unsigned char* out) {
    API_BEGIN
    render_on_host_bytes("debug_render_u8", device, sal, frames, n, H, W, cfg, offset, true, out);
    API_END
}

int p3d_debug_render_plan(int H, int W, int n, int contour_thickness, int offset, int* rows_per_block, int* cols_per_block,
                          int64_t* pixels_per_block) {
    API_BEGIN
    if (!rows_per_block || !cols_per_block || !pixels_per_block) throw P3dError("null argument");
    if (H < 1 || W < 1 || (long long)H * W > P3D_RENDER_MAX_PIXELS || n < 1 || n > 65535 || contour_thickness < 0 ||
        contour_thickness > P3D_RENDER_MAX_THICKNESS || offset < 0 || offset > 15)
        throw P3dError("debug_render_plan: 1 <= H * W <= 2^28, 1 .. 65535 maps, thickness 0 .. 4, offset in [0, 15]");
    const RenderPlan p = p3d_render_plan(H, W, contour_thickness);
    *rows_per_block = p.rows; *cols_per_block = p.cols; *pixels_per_block = p.chunk;
    API_END
}

int p3d_video_keep_source(p3d_handle* h, int on) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    h->video.keep_source(on);
    API_END
}

int p3d_video_source_info(p3d_handle* h, int* on, int* H0, int* W0, int64_t* bytes) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    h->video.need_open("video_source_info");
    if (on) *on = h->video.keep ? 1 : 0;
    if (H0) *H0 = h->video.H0;
    if (W0) *W0 = h->video.W0;
    if (bytes) *bytes = (int64_t)h->video.source.n;
    API_END
}

int p3d_video_render(p3d_handle* h, int first, int n, float scale, int H, int W, const unsigned char* frames, const p3d_render* cfg,
                     unsigned char* out, unsigned char* maps_out, double* stage_ms) {
    API_BEGIN
    const char* who = "video_render";
    if (!h) throw P3dError("null argument");
    h->video.need_open(who);
    // before the shape: a call that leaves the size to the source has none to name when there is no source
    if (!frames) need_kept_source(h, who);
    render_check(who, cfg, std::max(1, std::min(n, 65535)), H, W, out);
    RenderRequest r{who, n, H, W};
    r.cfg = cfg; r.frames = frames; r.out = out;
    video_stage_run<RenderStage>(h, r, first, scale, maps_out, stage_ms, 3, [&] {
        if (!frames) r.frames_dev = kept_source(h, who, first, n, H, W, "renders");
    });
    if (stage_ms && !frames) stage_ms[0] = 0.0;      // (nothing but the table went up)
    API_END
}

}  // extern "C"
namespace {
// ---- reframing around 8-bit maps (reframe.hip; the law in include/p3d_hip.h): one check, one launch description and one stage
// (the table of buffer sizes is its own) for p3d_reframe_u8, the video entry, p3d_debug_reframe_u8 and p3d_reframe_shots_u8 ---------
// What one reframing of n maps of H x W bytes asks for: frames on the host (uploaded), or on the device where they are (the kept
// source), or neither (tracks and masses only); track, raw, mass and out on the host, whatever is null is not copied back.
struct ReframeRequest {
    const char* who; int n, H, W;
    const p3d_reframe* cfg = nullptr;
    const unsigned char* frames = nullptr; const unsigned char* frames_dev = nullptr;
    int32_t* track = nullptr; int32_t* raw = nullptr; uint32_t* mass = nullptr; unsigned char* out = nullptr;
    bool timed = false;
    const int32_t* starts = nullptr; int n_shots = 0;      // host: a shot table in frames of the call (shots_table_check has passed it), or none
};
// The launches of reframe.hip behind some device bytes, with no arrival counters: they hand results to one another from launch to
// launch.  reframe_check has passed cfg and the shape before one is built.
struct ReframeStage : ByteStage {
    const ReframeRequest r;
    ReframeArgs a;
    unsigned char* df = nullptr;
    ShotTable shots;
    explicit ReframeStage(const ReframeRequest& r);
    bool crops() const { return r.out != nullptr; }
    void carve(Carve& c) override;
    void upload(hipStream_t s) override;
    void launch(hipStream_t s, const unsigned char* sal, unsigned*) override;
    void results(hipStream_t s) override;
};
void reframe_check(const char* who, const p3d_reframe* cfg, int n, int H, int W, const void* track) {
    if (!cfg || !track) throw P3dError("null argument");
    map_shape_check(who, n, H, W, P3D_REFRAME_MAX_PIXELS, "2^23, the bound that keeps a mass in 32 bits");
    if (cfg->crop_h < 1 || cfg->crop_h > H || cfg->crop_w < 1 || cfg->crop_w > W)
        throw P3dError(std::string(who) + ": the window is " + std::to_string(cfg->crop_h) + " x " + std::to_string(cfg->crop_w) + ", the map " +
                       std::to_string(H) + " x " + std::to_string(W) + "; 1 <= crop_h <= H and 1 <= crop_w <= W");
    if (cfg->gate < 0 || cfg->gate > 255) throw P3dError(std::string(who) + ": the gate is a level, 0 .. 255");
    if (cfg->smooth_radius < 0 || cfg->smooth_radius > 255) throw P3dError(std::string(who) + ": the smoothing radius is 0 .. 255 frames");
}
ReframeArgs reframe_args(const p3d_reframe& cfg, int n, int H, int W) {
    ReframeArgs a;
    a.n = n; a.H = H; a.W = W; a.hc = cfg.crop_h; a.wc = cfg.crop_w; a.gate = cfg.gate; a.radius = cfg.smooth_radius;
    const ReframePlan p = p3d_reframe_plan(H, W, a.hc, a.wc, n);
    a.maps_per_chunk = p.maps_per_chunk; a.search_blocks = p.search_blocks;
    return a;
}
// Elements of the buffers of one reframing
struct ReframeSizes {
    size_t sal, bgr, crop, pairs, masses, sat, best, part;
    explicit ReframeSizes(const ReframeArgs& a)
        : sal((size_t)a.n * (size_t)a.H * (size_t)a.W), bgr(sal * 3), crop((size_t)a.n * (size_t)a.hc * (size_t)a.wc * 3), pairs((size_t)a.n * 2),
          masses((size_t)a.n * 3) {
        const ReframePlan p = p3d_reframe_plan(a.H, a.W, a.hc, a.wc, a.n);
        sat = (size_t)p.sat_elems; best = (size_t)p.best_elems; part = (size_t)p.part_elems;
    }
};

ReframeStage::ReframeStage(const ReframeRequest& r_) : ByteStage(r_), r(r_), a(reframe_args(*r_.cfg, r_.n, r_.H, r_.W)), shots{r_.starts, r_.n_shots} {}
void ReframeStage::carve(Carve& c) {
    const ReframeSizes z(a);
    df = crops() && r.frames ? c.input<unsigned char>(z.bgr, 3) : nullptr;
    a.out = crops() ? c.take<unsigned char>(z.crop, 5) : nullptr;
    a.track = c.take<int32_t>(z.pairs);
    a.raw = c.take<int32_t>(z.pairs);
    a.mass = c.take<uint32_t>(z.masses);
    a.sat = c.take<unsigned>(z.sat);
    a.best = c.take<unsigned>(z.best);
    a.part = c.take<unsigned>(z.part);
    shots.carve(c);
}
void ReframeStage::upload(hipStream_t s) {
    if (df) HIPCHECK(hipMemcpyAsync(df, r.frames, ReframeSizes(a).bgr, hipMemcpyHostToDevice, s));
    shots.upload(s);
}
void ReframeStage::launch(hipStream_t s, const unsigned char* sal, unsigned*) {
    a.sal = sal; a.frames = !crops() ? nullptr : df ? df : r.frames_dev;
    shots.bind(a);
    HIPCHECK(p3d_reframe_launch(a, s));
}
void ReframeStage::results(hipStream_t s) {
    const ReframeSizes z(a);
    HIPCHECK(hipMemcpyAsync(r.track, a.track, z.pairs * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (r.raw) HIPCHECK(hipMemcpyAsync(r.raw, a.raw, z.pairs * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (r.mass) HIPCHECK(hipMemcpyAsync(r.mass, a.mass, z.masses * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (crops()) HIPCHECK(hipMemcpyAsync(r.out, a.out, z.crop, hipMemcpyDeviceToHost, s));
}
// The stage behind the host's bytes, for the three entries: p3d_reframe_u8 (no shot table, no offset), p3d_debug_reframe_u8 (no
// shot table, offset in [0, 15]) and p3d_reframe_shots_u8 (a shot table always, offset in [0, 15] or -1 for the stream's scratch)
enum ReframeEntry { REFRAME_OP, REFRAME_HOOK, REFRAME_SHOTS };
void reframe_on_host_bytes(ReframeEntry entry, const char* who, int device, const unsigned char* sal, const unsigned char* frames, int n, int H,
                           int W, const p3d_reframe* cfg, const int32_t* starts, int n_shots, int offset, int32_t* track, int32_t* raw,
                           uint32_t* mass, unsigned char* out) {
    const bool hook = entry != REFRAME_OP, shots = entry == REFRAME_SHOTS;
    if (!sal) throw P3dError("null argument");
    reframe_check(who, cfg, n, H, W, track);
    if ((frames == nullptr) != (out == nullptr)) throw P3dError(std::string(who) + ": out is given exactly when frames are");
    if (shots) shots_table_check(who, starts, n_shots, n);
    if (hook) offset_check(who, offset, shots);
    metric_args(device, sal, cfg, 1, 1, track);
    ReframeRequest r{who, n, H, W};
    r.cfg = cfg; r.frames = frames; r.track = track; r.raw = raw; r.mass = mass; r.out = out; r.starts = starts; r.n_shots = n_shots;
    ReframeStage stage(r);
    stage_on_host_bytes(stage, sal, hook ? offset : -1);
}
}  // namespace
extern "C" {

int p3d_reframe_u8(int device, const unsigned char* sal, const unsigned char* frames, int n, int H, int W, const p3d_reframe* cfg,
                   int32_t* track, int32_t* raw, uint32_t* mass, unsigned char* out) {
    API_BEGIN
    reframe_on_host_bytes(REFRAME_OP, "reframe_u8", device, sal, frames, n, H, W, cfg, nullptr, 0, -1, track, raw, mass, out);
    API_END
}

int p3d_debug_reframe_u8(int device, const unsigned char* sal, const unsigned char* frames, int n, int H, int W, const p3d_reframe* cfg,
                         int offset, int32_t* track, int32_t* raw, uint32_t* mass, unsigned char* out) {
    API_BEGIN
    reframe_on_host_bytes(REFRAME_HOOK, "debug_reframe_u8", device, sal, frames, n, H, W, cfg, nullptr, 0, offset, track, raw, mass, out);
    API_END
}

int p3d_reframe_shots_u8(int device, const unsigned char* sal, const unsigned char* frames, int n, int H, int W, const p3d_reframe* cfg,
                         const int32_t* starts, int n_shots, int offset, int32_t* track, int32_t* raw, uint32_t* mass, unsigned char* out) {
    API_BEGIN
    reframe_on_host_bytes(REFRAME_SHOTS, "reframe_shots_u8", device, sal, frames, n, H, W, cfg, starts, n_shots, offset, track, raw, mass, out);
    API_END
}

int p3d_debug_reframe_plan(int H, int W, int crop_h, int crop_w, int n, int* positions_per_block, int* search_blocks, int* maps_per_chunk,
                           int64_t* scratch_bytes) {
    API_BEGIN
    if (!positions_per_block || !search_blocks || !maps_per_chunk || !scratch_bytes) throw P3dError("null argument");
    if (H < 1 || W < 1 || (long long)H * W > P3D_REFRAME_MAX_PIXELS || n < 1 || n > 65535 || crop_h < 1 || crop_h > H || crop_w < 1 || crop_w > W)
        throw P3dError("debug_reframe_plan: 1 <= H * W <= 2^23, 1 .. 65535 maps, a window inside the map");
    const ReframePlan p = p3d_reframe_plan(H, W, crop_h, crop_w, n);
    *positions_per_block = p.positions_per_block; *search_blocks = p.search_blocks; *maps_per_chunk = p.maps_per_chunk;
    *scratch_bytes = (int64_t)p.scratch_bytes;
    API_END
}

int p3d_video_reframe(p3d_handle* h, int first, int n, float scale, int H, int W, const unsigned char* frames, const p3d_reframe* cfg,
                      int32_t* track, int32_t* raw, uint32_t* mass, unsigned char* out, unsigned char* maps_out, double* stage_ms) {
    API_BEGIN
    const char* who = "video_reframe";
    if (!h) throw P3dError("null argument");
    h->video.need_open(who);
    if (frames && !out) throw P3dError(std::string(who) + ": frames are given but no out to receive the windows");
    // before the shape: a call that leaves the size to the source has none to name when there is no source
    if (out && !frames) need_kept_source(h, who);
    reframe_check(who, cfg, std::max(1, std::min(n, 65535)), H, W, track);
    ReframeRequest r{who, n, H, W};
    r.cfg = cfg; r.frames = frames; r.track = track; r.raw = raw; r.mass = mass; r.out = out;
    std::vector<int32_t> shots;                            // the installed table in frames of the call: its shots cut the track's filter
    video_stage_run<ReframeStage>(h, r, first, scale, maps_out, stage_ms, 3, [&] {
        if (out && !frames) r.frames_dev = kept_source(h, who, first, n, H, W, "reframes");
        video_shots_into(h, first, shots, r);
    });
    if (stage_ms && !frames) stage_ms[0] = 0.0;      // (nothing went up)
    API_END
}

}  // extern "C"
namespace {
// ---- salient regions of 8-bit maps (regions.hip; the law in include/p3d_hip.h): one check, one launch description and one stage
// (the table of buffer sizes is its own) for p3d_regions_u8, the video entry and p3d_debug_regions_u8 -------------------------------
// What one labelling of n maps of H x W bytes asks for: regions, counts and labels on the host, whatever is null is not copied back.
struct RegionsCfg { int gate, connectivity, min_area, max_regions, link; };      // CONFIG's five ints under their names
struct RegionsRequest {
    const char* who; int n, H, W;
    const RegionsCfg* cfg = nullptr;
    int32_t* regions = nullptr; int32_t* counts = nullptr; unsigned char* labels = nullptr;
    bool timed = false;
    const int32_t* starts = nullptr; int n_shots = 0;      // host: a shot table in frames of the call (shots_table_check has passed it), or none
};
// The launches of regions.hip behind some device bytes, with no arrival counters: they hand results to one another from launch to
// launch.  regions_check has passed cfg and the shape before one is built.
struct RegionsStage : ByteStage {
    const RegionsRequest r;
    RegionsArgs a;
    ShotTable shots;
    explicit RegionsStage(const RegionsRequest& r);
    void carve(Carve& c) override;
    void upload(hipStream_t s) override;
    void launch(hipStream_t s, const unsigned char* sal, unsigned*) override;
    void results(hipStream_t s) override;
};
RegionsCfg regions_check(const char* who, const int* cfg5, int n, int H, int W, const void* regions) {
    if (!cfg5 || !regions) throw P3dError("null argument");
    const RegionsCfg parsed{cfg5[P3D_REGIONS_GATE], cfg5[P3D_REGIONS_CONNECTIVITY], cfg5[P3D_REGIONS_MIN_AREA], cfg5[P3D_REGIONS_MAX_REGIONS], cfg5[P3D_REGIONS_LINK]};
    const RegionsCfg* cfg = &parsed;
    map_shape_check(who, n, H, W, P3D_REGIONS_MAX_PIXELS, "2^23, the bound that keeps a mass in 32 bits");
    if (cfg->gate < 1 || cfg->gate > 255) throw P3dError(std::string(who) + ": the gate is a level, 1 .. 255");
    if (cfg->connectivity != 4 && cfg->connectivity != 8) throw P3dError(std::string(who) + ": the connectivity is 4 or 8, not " + std::to_string(cfg->connectivity));
    if (cfg->min_area < 1) throw P3dError(std::string(who) + ": the smallest area is at least 1 pixel");
    if (cfg->max_regions < 1 || cfg->max_regions > P3D_REGIONS_MAX)
        throw P3dError(std::string(who) + ": max_regions is 1 .. " + std::to_string(P3D_REGIONS_MAX) + ", not " + std::to_string(cfg->max_regions));
    if (cfg->link != 0 && cfg->link != 1) throw P3dError(std::string(who) + ": link is 0 or 1");
    return parsed;
}
RegionsArgs regions_args(const RegionsCfg& cfg, int n, int H, int W, bool labels) {
    RegionsArgs a;
    a.n = n; a.H = H; a.W = W; a.gate = cfg.gate; a.conn = cfg.connectivity; a.min_area = cfg.min_area; a.K = cfg.max_regions; a.link = cfg.link;
    a.lab_full = labels ? 1 : 0;
    const RegionsPlan p = p3d_regions_plan(H, W, n, a.K, a.link, a.lab_full);
    a.maps_per_chunk = p.maps_per_chunk; a.tiles_y = p.tiles_y; a.tiles_x = p.tiles_x; a.slots = p.slots;
    return a;
}
// Elements of the buffers of one labelling
struct RegionsSizes {
    size_t sal, records, counts; RegionsPlan p;
    explicit RegionsSizes(const RegionsArgs& a)
        : sal((size_t)a.n * (size_t)a.H * (size_t)a.W), records((size_t)a.n * (size_t)a.K * P3D_REGION_FIELDS), counts((size_t)a.n * 3),
          p(p3d_regions_plan(a.H, a.W, a.n, a.K, a.link, a.lab_full)) {}
};

RegionsStage::RegionsStage(const RegionsRequest& r_) : ByteStage(r_), r(r_), a(regions_args(*r_.cfg, r_.n, r_.H, r_.W, r_.labels != nullptr)),
      shots{r_.starts, r_.n_shots} {}
void RegionsStage::carve(Carve& c) {
    const RegionsSizes z(a);
    a.regions = c.take<int32_t>(z.records);
    a.counts = c.take<int32_t>(z.counts);
    a.parent = c.take<unsigned>((size_t)z.p.parent_elems);
    a.tab32 = c.take<unsigned>((size_t)z.p.tab32_elems);
    a.tab64 = c.take<unsigned long long>((size_t)z.p.tab64_elems);
    a.rank = c.take<unsigned char>((size_t)z.p.rank_elems);
    a.keys = c.take<unsigned long long>((size_t)z.p.key_elems);
    a.cnt = c.take<unsigned>((size_t)z.p.cnt_elems);
    a.ovl = z.p.ovl_elems ? c.take<unsigned>((size_t)z.p.ovl_elems) : nullptr;
    a.state = z.p.state_elems ? c.take<int32_t>((size_t)z.p.state_elems) : nullptr;
    a.lab = z.p.lab_elems ? c.take<unsigned char>((size_t)z.p.lab_elems, 5) : nullptr;
    shots.carve(c);
}
void RegionsStage::upload(hipStream_t s) { shots.upload(s); }
void RegionsStage::launch(hipStream_t s, const unsigned char* sal, unsigned*) {
    a.sal = sal;
    shots.bind(a);
    HIPCHECK(p3d_regions_launch(a, s));
}
void RegionsStage::results(hipStream_t s) {
    const RegionsSizes z(a);
    HIPCHECK(hipMemcpyAsync(r.regions, a.regions, z.records * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (r.counts) HIPCHECK(hipMemcpyAsync(r.counts, a.counts, z.counts * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (r.labels) HIPCHECK(hipMemcpyAsync(r.labels, a.lab, z.sal, hipMemcpyDeviceToHost, s));
}
// p3d_regions_u8 (offset < 0) and p3d_debug_regions_u8 (offset in [0, 15]): the stage behind the host's bytes
void regions_on_host_bytes(const char* who, int device, const unsigned char* sal, int n, int H, int W, const int* cfg, const int32_t* starts,
                           int n_shots, int offset, bool hook, int32_t* regions, int32_t* counts, unsigned char* labels) {
    if (!sal) throw P3dError("null argument");
    const RegionsCfg rc = regions_check(who, cfg, n, H, W, regions);
    if (starts || n_shots) shots_table_check(who, starts, n_shots, n);
    if (hook) offset_check(who, offset);
    metric_args(device, sal, cfg, 1, 1, regions);
    RegionsRequest r{who, n, H, W};
    r.cfg = &rc; r.regions = regions; r.counts = counts; r.labels = labels; r.starts = starts; r.n_shots = n_shots;
    RegionsStage stage(r);
    stage_on_host_bytes(stage, sal, hook ? offset : -1);
}
}  // namespace
extern "C" {

int p3d_regions_u8(int device, const unsigned char* sal, int n, int H, int W, const int cfg[5], const int32_t* starts, int n_shots,
                   int32_t* regions, int32_t* counts, unsigned char* labels) {
    API_BEGIN
    regions_on_host_bytes("regions_u8", device, sal, n, H, W, cfg, starts, n_shots, -1, false, regions, counts, labels);
    API_END
}

int p3d_debug_regions_u8(int device, const unsigned char* sal, int n, int H, int W, const int cfg[5], const int32_t* starts, int n_shots,
                         int offset, int32_t* regions, int32_t* counts, unsigned char* labels) {
    API_BEGIN
    regions_on_host_bytes("debug_regions_u8", device, sal, n, H, W, cfg, starts, n_shots, offset, true, regions, counts, labels);
    API_END
}

int p3d_debug_regions_plan(int H, int W, int n, int max_regions, int link, int labels, int* tile_h, int* tile_w, int* tiles_per_map,
                           int* maps_per_chunk, int64_t* scratch_bytes) {
    API_BEGIN
    if (!tile_h || !tile_w || !tiles_per_map || !maps_per_chunk || !scratch_bytes) throw P3dError("null argument");
    if (H < 1 || W < 1 || (long long)H * W > P3D_REGIONS_MAX_PIXELS || n < 1 || n > 65535 || max_regions < 1 || max_regions > P3D_REGIONS_MAX ||
        (link != 0 && link != 1) || (labels != 0 && labels != 1))
        throw P3dError("debug_regions_plan: 1 <= H * W <= 2^23, 1 .. 65535 maps, 1 .. 64 regions, link and labels 0 or 1");
    const RegionsPlan p = p3d_regions_plan(H, W, n, max_regions, link, labels);
    *tile_h = p.tile_h; *tile_w = p.tile_w; *tiles_per_map = p.tiles_y * p.tiles_x; *maps_per_chunk = p.maps_per_chunk;
    *scratch_bytes = (int64_t)p.scratch_bytes;
    API_END
}

int p3d_video_regions(p3d_handle* h, int first, int n, float scale, int H, int W, const int cfg[5], int32_t* regions, int32_t* counts,
                      unsigned char* labels, unsigned char* maps_out, double* stage_ms) {
    API_BEGIN
    const char* who = "video_regions";
    if (!h) throw P3dError("null argument");
    h->video.need_open(who);
    const RegionsCfg rc = regions_check(who, cfg, std::max(1, std::min(n, 65535)), H, W, regions);
    RegionsRequest r{who, n, H, W};
    r.cfg = &rc; r.regions = regions; r.counts = counts; r.labels = labels;
    std::vector<int32_t> shots;                            // the installed table in frames of the call, cut as p3d_video_reframe cuts it
    video_stage_run<RegionsStage>(h, r, first, scale, maps_out, stage_ms, 3, [&] { video_shots_into(h, first, shots, r); });
    if (stage_ms) stage_ms[0] = 0.0;                   // (nothing but a shot table went up)
    API_END
}

}  // extern "C"
namespace {
// ---- QP maps of 8-bit maps (qpmap.hip; the law in include/p3d_hip.h): one check, one launch description and one stage (the table of
// buffer sizes is its own) for p3d_qpmap_u8, the video entry and p3d_debug_qpmap_u8 -------------------------------------------------
// What one QP-map call on n maps of H x W bytes asks for: qp, levels and stats on the host, whatever is null is not copied back.
struct QpmapCfg { int block, peak_weight, dilate, fall, rise, balance, target, lo, hi; };      // CONFIG's nine ints under their names
struct QpmapRequest {
    const char* who; int n, H, W;
    const QpmapCfg* cfg = nullptr; const int32_t* law = nullptr;      // host: 256 entries (qpmap_check has passed them)
    int32_t* qp = nullptr; unsigned char* levels = nullptr; int32_t* stats = nullptr;
    bool timed = false;
    const int32_t* starts = nullptr; int n_shots = 0;      // host: a shot table in frames of the call (shots_table_check has passed it), or none
};
// qpmap.hip's launch sequence as a stage queues it: the launch arguments, the law and the optional shot table on the device, and
// the scratch of the first levels.  The qpmap stage holds one, and so does the prefilter stage, whose strength grid is these launches'
// qp: each carves it among its own buffers.
struct QpmapLaunches {
    QpmapArgs a;
    const int32_t* law; int32_t* dlaw = nullptr; ShotTable shots;
    QpmapLaunches(const QpmapCfg& c, int n, int H, int W, const int32_t* law, const int32_t* starts, int n_shots);
    size_t grid() const { return (size_t)a.n * (size_t)a.Hb * (size_t)a.Wb; }      // elements of qp and of levels
    void carve(Carve& c, bool levels, bool stats);         // qp, levels and stats where asked for, the scratch, the law, the shot table
    void upload(hipStream_t s) const;
    void launch(hipStream_t s, const unsigned char* sal);
};
// The launches of qpmap.hip behind some device bytes, with no arrival counters: they hand results to one another from launch to
// launch.  qpmap_check has passed cfg, the law and the shape before one is built.
struct QpmapStage : ByteStage {
    const QpmapRequest r;
    QpmapLaunches q;
    explicit QpmapStage(const QpmapRequest& r);
    void carve(Carve& c) override;
    void upload(hipStream_t s) override;
    void launch(hipStream_t s, const unsigned char* sal, unsigned*) override;
    void results(hipStream_t s) override;
};
QpmapCfg qpmap_check(const char* who, const int* cfg9, const int32_t* law, int n, int H, int W, const void* qp) {
    if (!cfg9 || !law || !qp) throw P3dError("null argument");
    const QpmapCfg c{cfg9[P3D_QPMAP_BLOCK], cfg9[P3D_QPMAP_PEAK_WEIGHT], cfg9[P3D_QPMAP_DILATE], cfg9[P3D_QPMAP_FALL], cfg9[P3D_QPMAP_RISE],
                     cfg9[P3D_QPMAP_BALANCE], cfg9[P3D_QPMAP_TARGET], cfg9[P3D_QPMAP_LO], cfg9[P3D_QPMAP_HI]};
    map_shape_check(who, n, H, W, P3D_QPMAP_MAX_PIXELS, "2^23, the bound that keeps an area-weighted sum of offsets in 32 bits");
    if (!block_size_ok(c.block))
        throw P3dError(std::string(who) + ": the block is 8, 16, 32, 64 or 128, not " + std::to_string(c.block));
    if (c.peak_weight < 0 || c.peak_weight > 256) throw P3dError(std::string(who) + ": peak_weight is 0 .. 256");
    if (c.dilate < 0 || c.dilate > 8) throw P3dError(std::string(who) + ": dilate is 0 .. 8 blocks");
    if (c.fall < 0 || c.fall > 254 || c.rise < 0 || c.rise > 254) throw P3dError(std::string(who) + ": fall and rise are 0 .. 254 (0: unlimited)");
    if (c.balance != 0 && c.balance != 1) throw P3dError(std::string(who) + ": balance is 0 or 1");
    if (c.lo < -127 || c.hi > 127 || c.lo > c.hi) throw P3dError(std::string(who) + ": -127 <= lo <= hi <= 127");
    if (c.target < c.lo || c.target > c.hi) throw P3dError(std::string(who) + ": the target lies in [lo, hi]");
    for (int v = 0; v < 256; ++v)
        if (law[v] < -127 || law[v] > 127) throw P3dError(std::string(who) + ": law[" + std::to_string(v) + "] = " + std::to_string(law[v]) + " is outside -127 .. 127");
    return c;
}
QpmapArgs qpmap_args(const QpmapCfg& c, int n, int H, int W) {
    QpmapArgs a;
    a.n = n; a.H = H; a.W = W; a.block = c.block; a.peak_weight = c.peak_weight; a.dilate = c.dilate; a.fall = c.fall; a.rise = c.rise;
    a.balance = c.balance; a.target = c.target; a.lo = c.lo; a.hi = c.hi;
    const QpmapPlan p = p3d_qpmap_plan(H, W, c.block, n);
    a.maps_per_chunk = p.maps_per_chunk; a.Hb = p.Hb; a.Wb = p.Wb; a.tiles_x = p.tiles_x;
    return a;
}
// Elements of the buffers of one call
struct QpmapSizes {
    size_t sal, grid, stats, lev0;
    explicit QpmapSizes(const QpmapArgs& a)
        : sal((size_t)a.n * (size_t)a.H * (size_t)a.W), grid((size_t)a.n * (size_t)a.Hb * (size_t)a.Wb), stats((size_t)a.n * 4),
          lev0((size_t)p3d_qpmap_plan(a.H, a.W, a.block, a.n).lev0_elems) {}
};

QpmapLaunches::QpmapLaunches(const QpmapCfg& c, int n, int H, int W, const int32_t* law_, const int32_t* starts, int n_shots)
    : a(qpmap_args(c, n, H, W)), law(law_), shots{starts, n_shots} {}
void QpmapLaunches::carve(Carve& c, bool levels, bool stats) {
    const QpmapSizes z(a);
    a.qp = c.take<int32_t>(z.grid);
    a.levels = levels ? c.take<unsigned char>(z.grid, 5) : nullptr;
    a.stats = stats ? c.take<int32_t>(z.stats) : nullptr;
    a.lev0 = c.take<unsigned char>(z.lev0);
    dlaw = c.input<int32_t>(256);
    shots.carve(c);
}
void QpmapLaunches::upload(hipStream_t s) const {
    HIPCHECK(hipMemcpyAsync(dlaw, law, 256 * sizeof(int32_t), hipMemcpyHostToDevice, s));
    shots.upload(s);
}
void QpmapLaunches::launch(hipStream_t s, const unsigned char* sal) {
    a.sal = sal; a.law = dlaw;
    shots.bind(a);
    HIPCHECK(p3d_qpmap_launch(a, s));
}
QpmapStage::QpmapStage(const QpmapRequest& r_) : ByteStage(r_), r(r_), q(*r_.cfg, r_.n, r_.H, r_.W, r_.law, r_.starts, r_.n_shots) {}
void QpmapStage::carve(Carve& c) { q.carve(c, r.levels != nullptr, r.stats != nullptr); }
void QpmapStage::upload(hipStream_t s) { q.upload(s); }
void QpmapStage::launch(hipStream_t s, const unsigned char* sal, unsigned*) { q.launch(s, sal); }
void QpmapStage::results(hipStream_t s) {
    const QpmapSizes z(q.a);
    HIPCHECK(hipMemcpyAsync(r.qp, q.a.qp, z.grid * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (r.levels) HIPCHECK(hipMemcpyAsync(r.levels, q.a.levels, z.grid, hipMemcpyDeviceToHost, s));
    if (r.stats) HIPCHECK(hipMemcpyAsync(r.stats, q.a.stats, z.stats * sizeof(int32_t), hipMemcpyDeviceToHost, s));
}
// p3d_qpmap_u8 (offset < 0) and p3d_debug_qpmap_u8 (offset in [0, 15]): the stage behind the host's bytes
void qpmap_on_host_bytes(const char* who, int device, const unsigned char* sal, int n, int H, int W, const int* cfg, const int32_t* law,
                         const int32_t* starts, int n_shots, int offset, bool hook, int32_t* qp, unsigned char* levels, int32_t* stats) {
    if (!sal) throw P3dError("null argument");
    const QpmapCfg qc = qpmap_check(who, cfg, law, n, H, W, qp);
    if (starts || n_shots) shots_table_check(who, starts, n_shots, n);
    if (hook) offset_check(who, offset);
    metric_args(device, sal, cfg, 1, 1, qp);
    QpmapRequest r{who, n, H, W};
    r.cfg = &qc; r.law = law; r.qp = qp; r.levels = levels; r.stats = stats; r.starts = starts; r.n_shots = n_shots;
    QpmapStage stage(r);
    stage_on_host_bytes(stage, sal, hook ? offset : -1);
}
}  // namespace
extern "C" {

int p3d_qpmap_u8(int device, const unsigned char* sal, int n, int H, int W, const int cfg[9], const int32_t law[256], const int32_t* starts,
                 int n_shots, int32_t* qp, unsigned char* levels, int32_t* stats) {
    API_BEGIN
    qpmap_on_host_bytes("qpmap_u8", device, sal, n, H, W, cfg, law, starts, n_shots, -1, false, qp, levels, stats);
    API_END
}

int p3d_debug_qpmap_u8(int device, const unsigned char* sal, int n, int H, int W, const int cfg[9], const int32_t law[256],
                       const int32_t* starts, int n_shots, int offset, int32_t* qp, unsigned char* levels, int32_t* stats) {
    API_BEGIN
    qpmap_on_host_bytes("debug_qpmap_u8", device, sal, n, H, W, cfg, law, starts, n_shots, offset, true, qp, levels, stats);
    API_END
}

int p3d_debug_qpmap_plan(int H, int W, int block, int n, int* strip_rows, int* tile_cols, int* blocks_per_map, int* maps_per_chunk,
                         int64_t* scratch_bytes) {
    API_BEGIN
    if (!strip_rows || !tile_cols || !blocks_per_map || !maps_per_chunk || !scratch_bytes) throw P3dError("null argument");
    if (H < 1 || W < 1 || (long long)H * W > P3D_QPMAP_MAX_PIXELS || n < 1 || n > 65535 || !block_size_ok(block))
        throw P3dError("debug_qpmap_plan: 1 <= H * W <= 2^23, 1 .. 65535 maps, a block of 8, 16, 32, 64 or 128");
    const QpmapPlan p = p3d_qpmap_plan(H, W, block, n);
    *strip_rows = p.strip_rows; *tile_cols = p.tile_cols; *blocks_per_map = p.blocks_per_map; *maps_per_chunk = p.maps_per_chunk;
    *scratch_bytes = (int64_t)p.scratch_bytes;
    API_END
}

int p3d_video_qpmap(p3d_handle* h, int first, int n, float scale, int H, int W, const int cfg[9], const int32_t law[256], int32_t* qp,
                    unsigned char* levels, int32_t* stats, unsigned char* maps_out, double* stage_ms) {
    API_BEGIN
    const char* who = "video_qpmap";
    if (!h) throw P3dError("null argument");
    h->video.need_open(who);
    const QpmapCfg qc = qpmap_check(who, cfg, law, std::max(1, std::min(n, 65535)), H, W, qp);
    QpmapRequest r{who, n, H, W};
    r.cfg = &qc; r.law = law; r.qp = qp; r.levels = levels; r.stats = stats;
    std::vector<int32_t> shots;                            // the installed table in frames of the call, cut as p3d_video_reframe cuts it
    video_stage_run<QpmapStage>(h, r, first, scale, maps_out, stage_ms, 3, [&] { video_shots_into(h, first, shots, r); });
    if (stage_ms) stage_ms[0] = 0.0;                   // (nothing but the law and a shot table went up)
    API_END
}

}  // extern "C"
namespace {
// ---- pre-filtering frames by their 8-bit maps (prefilter.hip; the law in include/p3d_hip.h): one check, one launch description and
// one stage for p3d_prefilter_u8, the video entry and p3d_debug_prefilter_u8.  The strength grid is qpmap.hip's launches ------------
// What one pre-filtering of n frames of H x W pixels by their maps asks for: frames on the host (uploaded) or on the device where they
// are (the kept source); out and grid on the host, a null grid is not copied back.
struct PrefilterCfg { int block, peak_weight, dilate, fall, rise, radius, passes; };      // CONFIG's seven ints under their names
struct PrefilterRequest {
    const char* who; int n, H, W;
    const PrefilterCfg* cfg = nullptr; const int32_t* law = nullptr;      // host: 256 entries (prefilter_check has passed them)
    const unsigned char* frames = nullptr; const unsigned char* frames_dev = nullptr; unsigned char* out = nullptr; int32_t* grid = nullptr;
    bool timed = false;
    const int32_t* starts = nullptr; int n_shots = 0;      // host: a shot table in frames of the call (shots_table_check has passed it), or none
};
// The launches of qpmap.hip (the strength grid, on this stage's own scratch) and of prefilter.hip behind some device bytes, with no
// arrival counters.  prefilter_check has passed cfg, the law and the shape before one is built.
struct PrefilterStage : ByteStage {
    const PrefilterRequest r;
    QpmapLaunches q;
    PrefilterArgs a;
    unsigned char* df = nullptr;
    explicit PrefilterStage(const PrefilterRequest& r);
    size_t bgr() const { return bytes * 3; }              // the bytes of n frames, in or out
    void carve(Carve& c) override;
    void upload(hipStream_t s) override;
    void launch(hipStream_t s, const unsigned char* sal, unsigned*) override;
    void results(hipStream_t s) override;
};
PrefilterCfg prefilter_check(const char* who, const int* cfg7, const int32_t* law, int n, int H, int W, const void* out) {
    if (!cfg7 || !law || !out) throw P3dError("null argument");
    const PrefilterCfg c{cfg7[P3D_PREFILTER_BLOCK], cfg7[P3D_PREFILTER_PEAK_WEIGHT], cfg7[P3D_PREFILTER_DILATE], cfg7[P3D_PREFILTER_FALL],
                         cfg7[P3D_PREFILTER_RISE], cfg7[P3D_PREFILTER_RADIUS], cfg7[P3D_PREFILTER_PASSES]};
    map_shape_check(who, n, H, W, P3D_PREFILTER_MAX_PIXELS, "2^23, the bound of the strength grid's launches");
    if (!block_size_ok(c.block))
        throw P3dError(std::string(who) + ": the block is 8, 16, 32, 64 or 128, not " + std::to_string(c.block));
    if (c.peak_weight < 0 || c.peak_weight > 256) throw P3dError(std::string(who) + ": peak_weight is 0 .. 256");
    if (c.dilate < 0 || c.dilate > 8) throw P3dError(std::string(who) + ": dilate is 0 .. 8 blocks");
    if (c.fall < 0 || c.fall > 64 || c.rise < 0 || c.rise > 64) throw P3dError(std::string(who) + ": fall and rise are 0 .. 64 (0: unlimited)");
    if (c.radius < 1 || c.radius > P3D_PREFILTER_MAX_RADIUS) throw P3dError(std::string(who) + ": the radius is 1 .. 16 pixels");
    if (c.passes < 1 || c.passes > P3D_PREFILTER_MAX_PASSES) throw P3dError(std::string(who) + ": 1 .. 3 passes");
    for (int v = 0; v < 256; ++v)
        if (law[v] < 0 || law[v] > 64) throw P3dError(std::string(who) + ": law[" + std::to_string(v) + "] = " + std::to_string(law[v]) + " is outside 0 .. 64");
    return c;
}
// STRENGTH GRID: the QP maps' configuration whose qp is g
QpmapCfg prefilter_grid_cfg(const PrefilterCfg& c) { return QpmapCfg{c.block, c.peak_weight, c.dilate, c.fall, c.rise, 0, 0, 0, 64}; }
PrefilterArgs prefilter_args(const PrefilterCfg& c, int n, int H, int W) {
    PrefilterArgs a;
    a.n = n; a.H = H; a.W = W; a.block = c.block; a.radius = c.radius; a.passes = c.passes;
    const PrefilterPlan p = p3d_prefilter_plan(H, W, c.block, c.radius, c.passes, n);
    a.Hb = p.Hb; a.Wb = p.Wb; a.tiles_x = p.tiles_x; a.tiles_y = p.tiles_y; a.frames_per_chunk = p.frames_per_chunk; a.mul = p.mul; a.shift = p.shift;
    return a;
}

PrefilterStage::PrefilterStage(const PrefilterRequest& r_)
    : ByteStage(r_), r(r_), q(prefilter_grid_cfg(*r_.cfg), r_.n, r_.H, r_.W, r_.law, r_.starts, r_.n_shots), a(prefilter_args(*r_.cfg, r_.n, r_.H, r_.W)) {}
void PrefilterStage::carve(Carve& c) {
    df = r.frames ? c.input<unsigned char>(bgr(), 3) : nullptr;
    a.out = c.take<unsigned char>(bgr(), 5);
    q.carve(c, false, false);
    const PrefilterPlan p = p3d_prefilter_plan(a.H, a.W, a.block, a.radius, a.passes, a.n);
    for (int k = 0; k < 2; ++k) a.tmp[k] = k < a.passes - 1 ? c.take<unsigned char>((size_t)p.tmp_bytes) : nullptr;
}
void PrefilterStage::upload(hipStream_t s) {
    q.upload(s);
    if (df) HIPCHECK(hipMemcpyAsync(df, r.frames, bgr(), hipMemcpyHostToDevice, s));
}
void PrefilterStage::launch(hipStream_t s, const unsigned char* sal, unsigned*) {
    q.launch(s, sal);
    a.frames = df ? df : r.frames_dev; a.grid = q.a.qp;
    HIPCHECK(p3d_prefilter_launch(a, s));
}
void PrefilterStage::results(hipStream_t s) {
    HIPCHECK(hipMemcpyAsync(r.out, a.out, bgr(), hipMemcpyDeviceToHost, s));
    if (r.grid) HIPCHECK(hipMemcpyAsync(r.grid, q.a.qp, q.grid() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
}
// p3d_prefilter_u8 (offset < 0) and p3d_debug_prefilter_u8 (offset in [0, 15]): the stage behind the host's bytes
void prefilter_on_host_bytes(const char* who, int device, const unsigned char* sal, const unsigned char* frames, int n, int H, int W,
                             const int* cfg, const int32_t* law, const int32_t* starts, int n_shots, int offset, bool hook, unsigned char* out,
                             int32_t* grid) {
    if (!sal || !frames) throw P3dError("null argument");
    const PrefilterCfg pc = prefilter_check(who, cfg, law, n, H, W, out);
    if (starts || n_shots) shots_table_check(who, starts, n_shots, n);
    if (hook) offset_check(who, offset);
    metric_args(device, sal, cfg, 1, 1, out);
    PrefilterRequest r{who, n, H, W};
    r.cfg = &pc; r.law = law; r.frames = frames; r.out = out; r.grid = grid; r.starts = starts; r.n_shots = n_shots;
    PrefilterStage stage(r);
    stage_on_host_bytes(stage, sal, hook ? offset : -1);
}
}  // namespace
extern "C" {

int p3d_prefilter_u8(int device, const unsigned char* sal, const unsigned char* frames, int n, int H, int W, const int cfg[7],
                     const int32_t law[256], const int32_t* starts, int n_shots, unsigned char* out, int32_t* grid) {
    API_BEGIN
    prefilter_on_host_bytes("prefilter_u8", device, sal, frames, n, H, W, cfg, law, starts, n_shots, -1, false, out, grid);
    API_END
}

int p3d_debug_prefilter_u8(int device, const unsigned char* sal, const unsigned char* frames, int n, int H, int W, const int cfg[7],
                           const int32_t law[256], const int32_t* starts, int n_shots, int offset, unsigned char* out, int32_t* grid) {
    API_BEGIN
    prefilter_on_host_bytes("debug_prefilter_u8", device, sal, frames, n, H, W, cfg, law, starts, n_shots, offset, true, out, grid);
    API_END
}

int p3d_debug_prefilter_plan(int H, int W, int block, int radius, int passes, int n, int* tile_rows, int* tile_cols, int* halo, int* fused,
                             int* blocks_per_frame, int* frames_per_chunk, int64_t* scratch_bytes, uint32_t* mul, int* shift) {
    API_BEGIN
    if (!tile_rows || !tile_cols || !halo || !fused || !blocks_per_frame || !frames_per_chunk || !scratch_bytes || !mul || !shift)
        throw P3dError("null argument");
    if (H < 1 || W < 1 || (long long)H * W > P3D_PREFILTER_MAX_PIXELS || n < 1 || n > 65535 || !block_size_ok(block) || radius < 1 ||
        radius > P3D_PREFILTER_MAX_RADIUS || passes < 1 || passes > P3D_PREFILTER_MAX_PASSES)
        throw P3dError("debug_prefilter_plan: 1 <= H * W <= 2^23, 1 .. 65535 frames, a block of 8, 16, 32, 64 or 128, a radius of 1 .. 16, 1 .. 3 passes");
    const PrefilterPlan p = p3d_prefilter_plan(H, W, block, radius, passes, n);
    *tile_rows = p.tile_rows; *tile_cols = p.tile_cols; *halo = p.halo; *fused = p.fused; *blocks_per_frame = (int)p.blocks_per_frame;
    *frames_per_chunk = p.frames_per_chunk; *scratch_bytes = (int64_t)p.scratch_bytes; *mul = p.mul; *shift = p.shift;
    API_END
}

int p3d_video_prefilter(p3d_handle* h, int first, int n, float scale, int H, int W, const unsigned char* frames, const int cfg[7],
                        const int32_t law[256], unsigned char* out, int32_t* grid, unsigned char* maps_out, double* stage_ms) {
    API_BEGIN
    const char* who = "video_prefilter";
    if (!h) throw P3dError("null argument");
    h->video.need_open(who);
    // before the shape: a call that leaves the size to the source has none to name when there is no source
    if (!frames) need_kept_source(h, who);
    const PrefilterCfg pc = prefilter_check(who, cfg, law, std::max(1, std::min(n, 65535)), H, W, out);
    PrefilterRequest r{who, n, H, W};
    r.cfg = &pc; r.law = law; r.frames = frames; r.out = out; r.grid = grid;
    std::vector<int32_t> shots;                            // the installed table in frames of the call, cut as p3d_video_qpmap cuts it
    video_stage_run<PrefilterStage>(h, r, first, scale, maps_out, stage_ms, 3, [&] {
        if (!frames) r.frames_dev = kept_source(h, who, first, n, H, W, "filters");
        video_shots_into(h, first, shots, r);
    });
    if (stage_ms && !frames) stage_ms[0] = 0.0;      // (nothing but the law and a shot table went up)
    API_END
}

}  // extern "C"
namespace {
// ---- distortion of frames under their 8-bit maps (distortion.hip; the law in include/p3d_hip.h): one check, one launch description
// and one stage for p3d_distortion_u8, the video entry and p3d_debug_distortion_u8; the plan hook shares the check's ranges ---------
// What one comparison of n test frames of H x W pixels with their reference frames under their maps asks for: test on the host
// (uploaded); ref on the host (uploaded) or on the device where it is (the kept source); table and block_sse on the host, a null
// block_sse is neither made nor copied back.
struct DistortionCfg { int block, gate; };                 // CONFIG's two ints under their names
struct DistortionRequest {
    const char* who; int n, H, W;
    const DistortionCfg* cfg = nullptr; const int32_t* wlaw = nullptr;      // host: 256 entries (distortion_check has passed them)
    const unsigned char* ref = nullptr; const unsigned char* ref_dev = nullptr; const unsigned char* test = nullptr;
    int64_t* table = nullptr; int64_t* block_sse = nullptr;
    bool timed = false;
};
// The launches of distortion.hip behind some device bytes, with no arrival counters: the sums meet in the table through integer
// atomics.  distortion_check has passed cfg, the law and the shape before one is built.
struct DistortionStage : ByteStage {
    const DistortionRequest r;
    DistortionArgs a;
    unsigned char* dref = nullptr; unsigned char* dtest = nullptr; int32_t* dlaw = nullptr;
    explicit DistortionStage(const DistortionRequest& r);
    size_t bgr() const { return bytes * 3; }              // the bytes of n frames
    size_t grid() const { return (size_t)a.n * (size_t)a.Hb * (size_t)a.Wb; }      // elements of the block map
    void carve(Carve& c) override;
    void upload(hipStream_t s) override;
    void launch(hipStream_t s, const unsigned char* sal, unsigned*) override;
    void results(hipStream_t s) override;
};
bool distortion_block_ok(int b) { return b == 0 || block_size_ok(b); }
DistortionCfg distortion_check(const char* who, const int* cfg2, const int32_t* wlaw, int n, int H, int W, const void* test, const void* table,
                               const void* block_sse) {
    if (!cfg2 || !wlaw || !test || !table) throw P3dError("null argument");
    const DistortionCfg c{cfg2[P3D_DISTORTION_BLOCK], cfg2[P3D_DISTORTION_GATE]};
    map_shape_check(who, n, H, W, P3D_DISTORTION_MAX_PIXELS, "2^23, the bound of the 64-bit integer sums");
    if (!distortion_block_ok(c.block)) throw P3dError(std::string(who) + ": the block is 0 (no block map), 8, 16, 32, 64 or 128, not " + std::to_string(c.block));
    if (c.block == 0 && block_sse) throw P3dError(std::string(who) + ": a block map is given and the block is 0");
    if (c.gate < 0 || c.gate > 255) throw P3dError(std::string(who) + ": the gate is 0 .. 255 (0: off)");
    for (int v = 0; v < 256; ++v)
        if (wlaw[v] < 0 || wlaw[v] > 255) throw P3dError(std::string(who) + ": wlaw[" + std::to_string(v) + "] = " + std::to_string(wlaw[v]) + " is outside 0 .. 255");
    return c;
}
DistortionArgs distortion_args(const DistortionCfg& c, int n, int H, int W) {
    DistortionArgs a;
    a.n = n; a.H = H; a.W = W; a.block = c.block; a.gate = c.gate;
    const DistortionPlan p = p3d_distortion_plan(H, W, c.block, n);
    a.Hb = p.Hb; a.Wb = p.Wb; a.tiles_x = p.tiles_x; a.tiles_y = p.tiles_y; a.win_rows = p.win_rows; a.win_cols = p.win_cols;
    a.ssim_tiles_x = p.ssim_tiles_x; a.ssim_tiles_y = p.ssim_tiles_y;
    return a;
}

DistortionStage::DistortionStage(const DistortionRequest& r_) : ByteStage(r_), r(r_), a(distortion_args(*r_.cfg, r_.n, r_.H, r_.W)) {}
void DistortionStage::carve(Carve& c) {
    dref = r.ref ? c.input<unsigned char>(bgr(), 3) : nullptr;
    dtest = c.input<unsigned char>(bgr(), 5);
    dlaw = c.input<int32_t>(256);
    a.table = c.take<long long>((size_t)a.n * P3D_DISTORTION_RECORD);
    a.block_sse = r.block_sse ? c.take<long long>(grid()) : nullptr;
}
void DistortionStage::upload(hipStream_t s) {
    HIPCHECK(hipMemcpyAsync(dlaw, r.wlaw, 256 * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (dref) HIPCHECK(hipMemcpyAsync(dref, r.ref, bgr(), hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(dtest, r.test, bgr(), hipMemcpyHostToDevice, s));
}
void DistortionStage::launch(hipStream_t s, const unsigned char* sal, unsigned*) {
    a.sal = sal; a.ref = dref ? dref : r.ref_dev; a.test = dtest; a.wlaw = dlaw;
    HIPCHECK(p3d_distortion_launch(a, s));
}
void DistortionStage::results(hipStream_t s) {
    static_assert(sizeof(long long) == sizeof(int64_t), "the table's element");
    HIPCHECK(hipMemcpyAsync(r.table, a.table, (size_t)a.n * P3D_DISTORTION_RECORD * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    if (r.block_sse) HIPCHECK(hipMemcpyAsync(r.block_sse, a.block_sse, grid() * sizeof(int64_t), hipMemcpyDeviceToHost, s));
}
// p3d_distortion_u8 (offset < 0) and p3d_debug_distortion_u8 (offset in [0, 15]): the stage behind the host's bytes
void distortion_on_host_bytes(const char* who, int device, const unsigned char* sal, const unsigned char* ref, const unsigned char* test, int n,
                              int H, int W, const int* cfg, const int32_t* wlaw, int offset, bool hook, int64_t* table, int64_t* block_sse) {
    if (!sal || !ref) throw P3dError("null argument");
    const DistortionCfg dc = distortion_check(who, cfg, wlaw, n, H, W, test, table, block_sse);
    if (hook) offset_check(who, offset);
    metric_args(device, sal, cfg, 1, 1, table);
    DistortionRequest r{who, n, H, W};
    r.cfg = &dc; r.wlaw = wlaw; r.ref = ref; r.test = test; r.table = table; r.block_sse = block_sse;
    DistortionStage stage(r);
    stage_on_host_bytes(stage, sal, hook ? offset : -1);
}
}  // namespace
extern "C" {

int p3d_distortion_u8(int device, const unsigned char* sal, const unsigned char* ref, const unsigned char* test, int n, int H, int W,
                      const int cfg[2], const int32_t wlaw[256], int64_t* table, int64_t* block_sse) {
    API_BEGIN
    distortion_on_host_bytes("distortion_u8", device, sal, ref, test, n, H, W, cfg, wlaw, -1, false, table, block_sse);
    API_END
}

int p3d_debug_distortion_u8(int device, const unsigned char* sal, const unsigned char* ref, const unsigned char* test, int n, int H, int W,
                            const int cfg[2], const int32_t wlaw[256], int offset, int64_t* table, int64_t* block_sse) {
    API_BEGIN
    distortion_on_host_bytes("debug_distortion_u8", device, sal, ref, test, n, H, W, cfg, wlaw, offset, true, table, block_sse);
    API_END
}

int p3d_debug_distortion_plan(int H, int W, int block, int n, int* tile_rows, int* tile_cols, int* blocks_per_frame, int* window_rows,
                              int* window_cols, int64_t* scratch_bytes) {
    API_BEGIN
    if (!tile_rows || !tile_cols || !blocks_per_frame || !window_rows || !window_cols || !scratch_bytes) throw P3dError("null argument");
    if (H < 1 || W < 1 || (long long)H * W > P3D_DISTORTION_MAX_PIXELS || n < 1 || n > 65535 || !distortion_block_ok(block))
        throw P3dError("debug_distortion_plan: 1 <= H * W <= 2^23, 1 .. 65535 frames, a block of 0, 8, 16, 32, 64 or 128");
    const DistortionPlan p = p3d_distortion_plan(H, W, block, n);
    *tile_rows = p.tile_rows; *tile_cols = p.tile_cols; *blocks_per_frame = (int)p.blocks_per_frame; *window_rows = p.win_rows;
    *window_cols = p.win_cols; *scratch_bytes = (int64_t)p.scratch_bytes;
    API_END
}

int p3d_video_distortion(p3d_handle* h, int first, int n, float scale, int H, int W, const unsigned char* ref, const unsigned char* test,
                         const int cfg[2], const int32_t wlaw[256], int64_t* table, int64_t* block_sse, unsigned char* maps_out,
                         double* stage_ms) {
    API_BEGIN
    const char* who = "video_distortion";
    if (!h) throw P3dError("null argument");
    h->video.need_open(who);
    // before the shape: a call that leaves the size to the source has none to name when there is no source
    if (!ref) need_kept_source(h, who);
    const DistortionCfg dc = distortion_check(who, cfg, wlaw, std::max(1, std::min(n, 65535)), H, W, test, table, block_sse);
    DistortionRequest r{who, n, H, W};
    r.cfg = &dc; r.wlaw = wlaw; r.ref = ref; r.test = test; r.table = table; r.block_sse = block_sse;
    video_stage_run<DistortionStage>(h, r, first, scale, maps_out, stage_ms, 3, [&] {
        if (!ref) r.ref_dev = kept_source(h, who, first, n, H, W, "compares");
    });
    API_END
}

}  // extern "C"
namespace {
// ---- SPLIT SWEEP on 8-bit maps: AUC-Borji and shuffled AUC (score_auc_u8.hip; the law in include/p3d_hip.h): one check and one
// launch sequence, in the score stage (the table of buffer sizes is its own), for p3d_score_sweep_u8, p3d_video_score_auc and
// p3d_debug_score_sweep_u8 ------------------------------------------------------------------------------------------------------------
ScoreSweepArgs sweep_args(const char* who, int n, long long n_pix, int n_rep, double step) {
    ScoreSweepArgs q;
    q.kmax = p3d_sweep_kmax(step);
    if (q.kmax < 1) throw P3dError(std::string(who) + ": the step is positive and gives at most 1024 thresholds (ceil(1 / step))");
    if (n_rep < 1) throw P3dError(std::string(who) + ": n_rep >= 1");
    q.n = n; q.n_pix = (int)n_pix; q.n_rep = n_rep; q.step = step; q.cols = p3d_sweep_cols(q.kmax, n_rep);
    return q;
}
struct SweepSizes {
    size_t lev, lad, info, per_rep;
    explicit SweepSizes(const ScoreSweepArgs& q)
        : lev((size_t)q.n * 256), lad((size_t)q.n * (q.kmax + 1)), info((size_t)q.n * 4), per_rep((size_t)q.n * q.n_rep) {}
};
// meta [n][2] of maps whose rows are concatenated: the row count, the offset of the first index; -> the number of indices
std::vector<long long> sweep_meta(const char* who, const int* n_rows, int n, int n_rep, size_t& total) {
    std::vector<long long> meta((size_t)n * 2);
    long long at = 0;
    for (int b = 0; b < n; ++b) {
        if (n_rows[b] < 0) throw P3dError(std::string(who) + ": map " + std::to_string(b) + ": a negative row count");
        meta[(size_t)b * 2] = n_rows[b]; meta[(size_t)b * 2 + 1] = at;
        at += (long long)n_rows[b] * n_rep;
        if (at > INT32_MAX) throw P3dError(std::string(who) + ": too many indices");
    }
    total = (size_t)at;
    return meta;
}
// fixated pixels (byte >= 128) of every map, counted on the host
std::vector<int> host_n_fix(const unsigned char* fixation, int n, long long n_pix) {
    std::vector<int> nf((size_t)n);
    for (int b = 0; b < n; ++b) {
        const unsigned char* p = fixation + (size_t)b * n_pix;
        int k = 0;
        for (long long i = 0; i < n_pix; ++i) k += p[i] >> 7;
        nf[(size_t)b] = k;
    }
    return nf;
}
// the op-level sweep's checks of its arguments and shapes
void sweep_op_shape(const char* who, const void* sal, const void* fixation, int n, int H, int W, const int* n_rows, const void* per_rep) {
    if (!sal || !fixation || !n_rows || !per_rep) throw P3dError("null argument");
    map_shape_check(who, n, H, W, P3D_SCORE_MAX_PIXELS, "2^23");
}
// the device's counts (info[b][0] = nf) against the rows: n_rows[b] <= nf[b]
void sweep_check_rows(const char* who, const std::vector<int>& info, const int* n_rows, int n) {
    for (int b = 0; b < n; ++b)
        if (n_rows[b] > info[(size_t)b * 4])
            throw P3dError(std::string(who) + ": map " + std::to_string(b) + ": " + std::to_string(n_rows[b]) + " rows, but the map has " +
                           std::to_string(info[(size_t)b * 4]) + " fixated pixels");
}

ScoreStage::ScoreStage(const ScoreRequest& r_)
    : ByteStage(r_), r(r_),
      a(score_args(r_.n, (long long)r_.H * r_.W, r_.flags, r_.flags ? r_.ties : P3D_SCORE_TIES_REFERENCE)), sweeps(r_.timed && (r_.borji || r_.shuffled), 2) {
    if (!sweep()) return;
    const long long N = (long long)r.H * r.W;
    q = sweep_args(r.who, r.n, N, r.n_rep, r.step);
    if ((r.borji && !r.idx_rows) || r.shuffled) {
        nf = host_n_fix(r.fixation, r.n, N);
        info.assign(SweepSizes(q).info, 0);
    }
    if (r.borji) {
        metaB = sweep_meta(r.who, r.idx_rows ? r.idx_rows : nf.data(), r.n, r.n_rep, totB);
        if (totB > 0 && !r.idx) throw P3dError("null argument");
        check_indices(r.idx, totB, N, r.who);
    }
    if (r.shuffled) {
        const p3d_handle* h = r.pool;
        h->fixpool.need_open(r.who);
        if (!h->fixpool.vu.begun) throw P3dError(std::string(r.who) + ": no union is held (p3d_video_shuffled_begin)");
        if (h->fixpool.H != r.H || h->fixpool.W != r.W)
            throw P3dError(std::string(r.who) + ": the fixation pool holds " + std::to_string(h->fixpool.H) + " x " + std::to_string(h->fixpool.W) + " maps, the call scores " +
                           std::to_string(r.H) + " x " + std::to_string(r.W));
        if (h->fixpool.vu.n != r.n) throw P3dError(std::string(r.who) + ": the union was taken for " + std::to_string(h->fixpool.vu.n) + " frames, the call scores " + std::to_string(r.n));
        for (int b = 0; b < r.n; ++b)
            if (r.n_rows[b] != (int)std::min<long long>(nf[(size_t)b], h->fixpool.vu.n_other[(size_t)b]))
                throw P3dError(std::string(r.who) + ": frame " + std::to_string(b) + ": n_rows = " + std::to_string(r.n_rows[b]) + ", but min(n_fix, n_other) = min(" +
                               std::to_string(nf[(size_t)b]) + ", " + std::to_string(h->fixpool.vu.n_other[(size_t)b]) + ")");
        p3d_handle::FixPool::check_draws(r.who, r.ranks, r.n_rows, h->fixpool.vu.n_other.data(), r.n, r.n_rep, r.step);
        metaS = sweep_meta(r.who, r.n_rows, r.n, r.n_rep, totS);
        meta3.assign((size_t)r.n * 3, 0);
        for (int b = 0; b < r.n; ++b) { meta3[(size_t)b * 3 + 2] = (int)metaS[(size_t)b * 2 + 1]; max_rows = std::max(max_rows, r.n_rows[b]); }
    }
}
size_t ScoreStage::counters() const { return ScoreSizes(a).counters; }
void ScoreStage::carve(Carve& c) {
    const ScoreSizes z(a);
    dd = r.density && r.flags ? c.input<unsigned char>(bytes, 2) : nullptr;
    dx = r.fixation ? c.input<unsigned char>(bytes, 3) : nullptr;
    a.tab = c.take<unsigned>(z.tab); a.lut = c.take<double>(z.lut); a.part = c.take<double>(z.part); a.out = c.take<double>(z.out);
    if (!sweep()) return;
    const SweepSizes w(q);
    q.lev = c.take<int>(w.lev); q.lad = c.take<unsigned>(w.lad); q.info = c.take<int>(w.info);
    if (r.borji) { didx = c.input<int>(totB); dmetaB = c.input<long long>(metaB.size()); perB = c.take<double>(w.per_rep); }
    if (r.top) dtop = c.take<int>(w.per_rep);
    if (r.shuffled) {
        dranks = c.input<int>(totS); dsel = c.take<int>(totS); dmeta3 = c.input<int>(meta3.size()); drows = c.input<int>((size_t)r.n);
        dmetaS = c.input<long long>(metaS.size()); perS = c.take<double>(w.per_rep);
    }
}
void ScoreStage::upload(hipStream_t s) {
    if (dd) HIPCHECK(hipMemcpyAsync(dd, r.density, bytes, hipMemcpyHostToDevice, s));
    if (dx) HIPCHECK(hipMemcpyAsync(dx, r.fixation, bytes, hipMemcpyHostToDevice, s));
    if (r.borji) {
        if (totB) HIPCHECK(hipMemcpyAsync(didx, r.idx, totB * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHECK(hipMemcpyAsync(dmetaB, metaB.data(), metaB.size() * sizeof(long long), hipMemcpyHostToDevice, s));
    }
    if (r.shuffled) {
        if (totS) HIPCHECK(hipMemcpyAsync(dranks, r.ranks, totS * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHECK(hipMemcpyAsync(dmeta3, meta3.data(), meta3.size() * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHECK(hipMemcpyAsync(drows, r.n_rows, (size_t)r.n * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHECK(hipMemcpyAsync(dmetaS, metaS.data(), metaS.size() * sizeof(long long), hipMemcpyHostToDevice, s));
    }
}
void ScoreStage::prepare(hipStream_t s, const unsigned char* sal, unsigned* counters) {
    a.sal = sal; a.den = dd; a.fix = dx; a.counter = counters;
    score_sequence(a, s);                                 // pass A once, for the columns and for the sweeps
    sweeps.mark(0, s);
    if (!sweep()) return;
    q.sal = sal; q.tab = a.tab;
    HIPCHECK(p3d_sweep_launch(SWEEP_PREP, q, s));
}
void ScoreStage::launch(hipStream_t s, const unsigned char* sal, unsigned* counters) {
    prepare(s, sal, counters);
    if (r.rows_checked) {
        std::vector<int> nf_dev(SweepSizes(q).info);
        HIPCHECK(hipDeviceSynchronize());
        HIPCHECK(copy_now(nf_dev.data(), q.info, nf_dev.size() * sizeof(int), hipMemcpyDeviceToHost, s));      // nf, read back once
        sweep_check_rows(r.who, nf_dev, r.idx_rows, r.n);
    }
    sweep_rest(s);
}
void ScoreStage::sweep_rest(hipStream_t s) {
    if (r.borji) {
        q.idx = didx; q.meta = dmetaB; q.per_rep = perB; q.top = dtop;
        HIPCHECK(p3d_sweep_launch(SWEEP_RUN, q, s));
    }
    if (r.shuffled) {
        const p3d_handle* h = r.pool;
        if (totS) {
            FixSelectArgs e;
            e.uni = h->fixpool.vu.uni; e.prefix = h->fixpool.vu.prefix; e.bsum = h->fixpool.vu.bsum; e.n_other = h->fixpool.vu.n_other_dev; e.nw = h->fixpool.nw; e.B = r.n;
            e.nsb = p3d_fix_scan_blocks(h->fixpool.nw); e.n_rep = r.n_rep; e.max_rows = max_rows; e.meta = dmeta3; e.n_rows = drows; e.ranks = dranks; e.out = dsel;
            HIPCHECK(p3d_fix_select_launch(e, s));
        }
        ScoreSweepArgs qs = q;
        qs.idx = dsel; qs.meta = dmetaS; qs.per_rep = perS; qs.top = nullptr;
        HIPCHECK(p3d_sweep_launch(SWEEP_RUN, qs, s));
    }
    sweeps.mark(1, s);
}
void ScoreStage::results(hipStream_t s) {
    if (r.flags) HIPCHECK(hipMemcpyAsync(r.out, a.out, ScoreSizes(a).out * sizeof(double), hipMemcpyDeviceToHost, s));
    if (!sweep()) return;
    const SweepSizes w(q);
    if (r.borji) HIPCHECK(hipMemcpyAsync(r.borji, perB, w.per_rep * sizeof(double), hipMemcpyDeviceToHost, s));
    if (dtop) HIPCHECK(hipMemcpyAsync(r.top, dtop, w.per_rep * sizeof(int), hipMemcpyDeviceToHost, s));
    if (r.shuffled) HIPCHECK(hipMemcpyAsync(r.shuffled, perS, w.per_rep * sizeof(double), hipMemcpyDeviceToHost, s));
    if (!nf.empty()) HIPCHECK(hipMemcpyAsync(info.data(), q.info, info.size() * sizeof(int), hipMemcpyDeviceToHost, s));      // (to hold against the host's)
}
void ScoreStage::check_counts() const {
    for (size_t b = 0; b < nf.size(); ++b)
        if (info[b * 4] != nf[b])
            throw P3dError(std::string(r.who) + ": frame " + std::to_string(b) + ": the device counted " + std::to_string(info[b * 4]) + " fixated pixels, the host " +
                           std::to_string(nf[b]));
}
// p3d_video_score and p3d_video_score_auc behind the checks of their arguments.  stage_ms (null, or n_ms = 3 or 4 values): uploads,
// the chain, the launches less the sweeps, the sweeps.
void video_score_run(p3d_handle* h, int first, float scale, ScoreRequest r, unsigned char* maps_out, double* stage_ms, int n_ms) {
    HIPCHECK(hipSetDevice(h->cfg.device));
    const VideoSource src(h, r.who, first, r.n, true, 65535);
    r.timed = stage_ms != nullptr;
    ScoreStage stage(r);
    for (int i = 0; stage_ms && i < n_ms; ++i) stage_ms[i] = 0.0;
    maps_u8_chain(h, r.n, h->pred->H, h->pred->W, scale, r.H, r.W, maps_out, nullptr, src.extra(), src, &stage);
    if (stage_ms) {
        const double sw = stage.sweep_ms();
        stage_ms[0] = stage.ms[0]; stage_ms[1] = stage.ms[1]; stage_ms[2] = std::max(0.0, stage.ms[2] - sw);
        if (n_ms > 3) stage_ms[3] = sw;
    }
    stage.check_counts();
}
}  // namespace
extern "C" {

int p3d_score_sweep_u8(int device, const unsigned char* sal, const unsigned char* fixation, int n, int H, int W, const int* idx,
                       const int* n_rows, int n_rep, double step, double* per_rep) {
    API_BEGIN
    const char* who = "score_sweep_u8";
    sweep_args(who, n, (long long)H * W, n_rep, step);      // (the step and n_rep are refused first, as in the hook)
    sweep_op_shape(who, sal, fixation, n, H, W, n_rows, per_rep);
    ScoreRequest r{who, n, H, W};
    r.fixation = fixation; r.idx = idx; r.idx_rows = n_rows; r.borji = per_rep; r.n_rep = n_rep; r.step = step; r.rows_checked = true;
    ScoreStage stage(r);
    metric_args(device, sal, fixation, 1, 1, per_rep);
    stage_on_host_bytes(stage, sal);
    API_END
}

int p3d_debug_score_sweep_u8(int device, const unsigned char* sal, const unsigned char* fixation, int n, int H, int W, const int* idx,
                             const int* n_rows, int n_rep, double step, int offset, int* lev_out, int* top_out, double* per_rep) {
    API_BEGIN
    const char* who = "debug_score_sweep_u8";
    sweep_args(who, n, (long long)H * W, n_rep, step);
    sweep_op_shape(who, sal, fixation, n, H, W, n_rows, per_rep);
    ScoreRequest r{who, n, H, W};
    r.fixation = fixation; r.idx = idx; r.idx_rows = n_rows; r.borji = per_rep; r.n_rep = n_rep; r.step = step; r.rows_checked = true;
    r.top = top_out;
    ScoreStage stage(r);
    if (!lev_out || !top_out) throw P3dError("null argument");
    offset_check(who, offset);
    metric_args(device, sal, fixation, 1, 1, per_rep);
    stage_on_host_bytes(stage, sal, offset, [&](const GuardedRun& g) {
        g.read(stage.q.lev, lev_out);
        g.unchanged(stage.a.lut); g.unchanged(stage.a.part);      // no pass B: nothing of its was written
        g.counters_at_zero();
    });
    API_END
}

int p3d_video_shuffled_begin(p3d_handle* h, int n, const int* ids, int M, uint32_t* n_other_out) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->video_shuffled_begin(ids, n, M, n_other_out);
    API_END
}

int p3d_video_score(p3d_handle* h, int first, int n, float scale, int H, int W, const unsigned char* density, const unsigned char* fixation,
                    int flags, int ties, double* out, unsigned char* maps_out, double* stage_ms) {
    API_BEGIN
    if (!h) throw P3dError("null argument");
    score_check("video_score", density, fixation, std::max(1, std::min(n, 65535)), H, W, flags, ties, out);
    ScoreRequest r{"video_score", n, H, W};
    r.flags = flags; r.ties = ties; r.density = density; r.fixation = fixation; r.out = out;
    video_score_run(h, first, scale, r, maps_out, stage_ms, 3);
    API_END
}

int p3d_video_score_auc(p3d_handle* h, int first, int n, float scale, int H, int W, const unsigned char* density, const unsigned char* fixation,
                        int flags, int ties, double* out, const int* borji_idx, const int* ranks, const int* n_rows, int n_rep, double step,
                        double* borji_per_rep, double* shuffled_per_rep, double* stage_ms) {
    API_BEGIN
    const char* who = "video_score_auc";
    if (!h) throw P3dError("null argument");
    const bool borji = borji_idx != nullptr, shuf = ranks != nullptr;
    const int nc = std::max(1, std::min(n, 65535));
    if (flags != 0) score_check(who, density, fixation, nc, H, W, flags, ties, out);
    else if (out) throw P3dError(std::string(who) + ": flags = 0 selects no column, so out must be NULL");
    if (flags == 0 && !borji && !shuf) throw P3dError(std::string(who) + ": nothing is asked for");
    map_shape_check(who, nc, H, W, P3D_SCORE_MAX_PIXELS, "2^23");
    if ((borji || shuf) && !fixation) throw P3dError(std::string(who) + ": AUC-Borji and shuffled AUC need the fixation maps");
    if ((borji && !borji_per_rep) || (shuf && (!n_rows || !shuffled_per_rep))) throw P3dError("null argument");
    ScoreRequest r{who, n, H, W};
    r.flags = flags; r.ties = ties; r.density = density; r.fixation = fixation; r.out = out; r.n_rep = n_rep; r.step = step;
    if (borji) { r.idx = borji_idx; r.borji = borji_per_rep; }
    if (shuf) { r.ranks = ranks; r.n_rows = n_rows; r.pool = h; r.shuffled = shuffled_per_rep; }
    video_score_run(h, first, scale, r, nullptr, stage_ms, 4);
    API_END
}

// The launches of video.hip from their launch descriptions, on host arrays.  Every device buffer sits `offset` elements past
// a 16-byte boundary between guard elements; a guard or an input that a launch changed is an error.
}  // extern "C"
namespace {
void video_hook_device(int device, int offset) {
    int ndev = 0;
    HIPCHECK(hipGetDeviceCount(&ndev));
    if (ndev <= 0) throw P3dError("no HIP device: libp3dhip has no CPU fallback");
    if (device < 0 || device >= ndev) throw P3dError("bad device ordinal");
    if (offset < 0 || offset > 3) throw P3dError("video hook: offset is 0 .. 3");
    HIPCHECK(hipSetDevice(device));
}
}  // namespace
extern "C" {

int p3d_debug_video_gather(int device, const float* store, int F, int T, int64_t frame_elems, const int* starts, int n_windows, int B,
                           int offset, float* x) {
    API_BEGIN
    if (!store || !starts || !x) throw P3dError("null argument");
    if (T < 1 || F < T || frame_elems < 1 || B < 1 || n_windows < 1 || n_windows > B) throw P3dError("video_gather: bad shape");
    if ((int64_t)F * frame_elems > (int64_t)1 << 31 || (int64_t)B * T * frame_elems > (int64_t)1 << 31) throw P3dError("video_gather: the hook takes up to 2^31 floats");
    video_hook_device(device, offset);
    std::vector<int> padded(starts, starts + n_windows);
    padded.resize((size_t)B, starts[n_windows - 1]);
    const int64_t ns = (int64_t)F * frame_elems, nx = (int64_t)B * T * frame_elems;
    Guarded<float> sb((size_t)ns, 8, (size_t)offset, store), xb((size_t)nx, 8, (size_t)offset, nullptr);
    DevArr<int> tab((size_t)B, padded.data());
    VideoGatherArgs a;
    a.store = sb.data(); a.x = xb.data(); a.starts = tab.p; a.starts_host = padded.data(); a.B = B; a.T = T; a.F = F; a.frame_elems = frame_elems;
    if (std::string(p3d_video_gather_desc(a).kernel) != "video_gather_kernel") throw P3dError("video_gather: launch description names another kernel");
    HIPCHECK(p3d_video_gather(a, nullptr));
    HIPCHECK(hipDeviceSynchronize());
    sb.unchanged("video_gather");
    xb.back(x, "video_gather");
    API_END
}

}  // extern "C"
namespace {
// p3d_debug_video_scatter and, with a shot table, p3d_debug_video_scatter_shots: the scatter launch of the plan of one call
void video_scatter_hook(int device, int mode, const float* pred, int B, int T, int64_t hw, int ld, const int32_t* shots, int n_shots,
                        const int* starts, int n_windows, int F, int last_start, float* store, int32_t* count, int offset) {
    if (!pred || !starts || !store || !count) throw P3dError("null argument");
    if (hw < 1 || ld < 1) throw P3dError("video_scatter: bad shape");
    const p3d_handle::Video::Plan p = p3d_handle::Video::plan(mode, F, T, B, last_start, count, nullptr, starts, n_windows, shots, n_shots);
    const int64_t np = (int64_t)B * T * hw * ld, ns = (int64_t)F * hw;
    if (np > (int64_t)1 << 31 || ns > (int64_t)1 << 31) throw P3dError("video_scatter: the hook takes up to 2^31 floats");
    video_hook_device(device, offset);
    Guarded<float> pb((size_t)np, 8, (size_t)offset, pred), sb((size_t)ns, 8, (size_t)offset, store);
    Guarded<int32_t> cb((size_t)F, 8, 0, count);
    if (!p.dst.empty()) {
        DevArr<P3dVideoDst> dst(p.dst.size(), p.dst.data());
        DevArr<int> src(p.src.size(), p.src.data());
        VideoScatterArgs a;
        a.mode = mode; a.pred = pb.data(); a.ld = ld; a.maps = B * T; a.hw = hw;
        a.store = sb.data(); a.count = cb.data(); a.F = F;
        a.dst = dst.p; a.src = src.p; a.dst_host = p.dst.data(); a.src_host = p.src.data();
        a.ndst = (int)p.dst.size(); a.nsrc = (int)p.src.size();
        if (std::string(p3d_video_scatter_desc(a).kernel) != "video_scatter_kernel<" + std::to_string(mode) + ">")
            throw P3dError("video_scatter: launch description names another kernel");
        HIPCHECK(p3d_video_scatter(a, nullptr));
        HIPCHECK(hipDeviceSynchronize());
    }
    pb.unchanged("video_scatter");
    std::vector<int32_t> co((size_t)F);
    cb.back(co.data(), "video_scatter");
    if (memcmp(co.data(), p.count.data(), (size_t)F * 4) != 0) throw P3dError("video_scatter: the device's counts differ from the plan's");
    sb.back(store, "video_scatter");
    memcpy(count, p.count.data(), (size_t)F * 4);
}
}  // namespace
extern "C" {

int p3d_debug_video_scatter(int device, int mode, const float* pred, int B, int T, int64_t hw, int ld, const int* starts, int n_windows,
                            int F, int last_start, float* store, int32_t* count, int offset) {
    API_BEGIN
    video_scatter_hook(device, mode, pred, B, T, hw, ld, nullptr, 0, starts, n_windows, F, last_start, store, count, offset);
    API_END
}

int p3d_debug_video_scatter_shots(int device, int mode, const float* pred, int B, int T, int64_t hw, int ld, const int32_t* shot_starts,
                                  int n_shots, const int* starts, int n_windows, int F, int last_start, float* store, int32_t* count,
                                  int offset) {
    API_BEGIN
    if (!shot_starts) throw P3dError("null argument");
    video_scatter_hook(device, mode, pred, B, T, hw, ld, shot_starts, n_shots, starts, n_windows, F, last_start, store, count, offset);
    API_END
}

int p3d_debug_video_gather_slots(int device, const float* store, int F, int T, int64_t frame_elems, const int32_t* shot_starts, int n_shots,
                                 const int* starts, int n_windows, int B, int offset, float* x) {
    API_BEGIN
    if (!store || !shot_starts || !starts || !x) throw P3dError("null argument");
    if (T < 1 || F < T || frame_elems < 1 || B < 1) throw P3dError("video_gather_slots: bad shape");
    if ((int64_t)F * frame_elems > (int64_t)1 << 31 || (int64_t)B * T * frame_elems > (int64_t)1 << 31) throw P3dError("video_gather_slots: the hook takes up to 2^31 floats");
    const std::vector<int32_t> none((size_t)F, 0);      // the windows as p3d_video_predict_shots validates them, every frame put
    const p3d_handle::Video::Plan p = p3d_handle::Video::plan(VIDEO_NEWEST, F, T, B, -1, none.data(), nullptr, starts, n_windows, shot_starts, n_shots);
    video_hook_device(device, offset);
    const int64_t ns = (int64_t)F * frame_elems, nx = (int64_t)B * T * frame_elems;
    Guarded<float> sb((size_t)ns, 8, (size_t)offset, store), xb((size_t)nx, 8, (size_t)offset, nullptr);
    DevArr<int> tab(p.slots.size(), p.slots.data());
    VideoGatherSlotsArgs a;
    a.store = sb.data(); a.x = xb.data(); a.frames = tab.p; a.frames_host = p.slots.data(); a.B = B; a.T = T; a.F = F; a.frame_elems = frame_elems;
    if (std::string(p3d_video_gather_slots_desc(a).kernel) != "video_gather_slots_kernel") throw P3dError("video_gather_slots: launch description names another kernel");
    HIPCHECK(p3d_video_gather_slots(a, nullptr));
    HIPCHECK(hipDeviceSynchronize());
    sb.unchanged("video_gather_slots");
    xb.back(x, "video_gather_slots");
    API_END
}

int p3d_debug_video_plan_shots(int mode, int F, int T, int B, int last_start, const int32_t* count_in, const int32_t* shot_starts, int n_shots,
                               const int* starts, int n_windows, int32_t* count_out, int* slots_out, int* live_out) {
    API_BEGIN
    if (!shot_starts || !count_out || !slots_out || !live_out) throw P3dError("null argument");
    const p3d_handle::Video::Plan p = p3d_handle::Video::plan(mode, F, T, B, last_start, count_in, nullptr, starts, n_windows, shot_starts, n_shots);
    memcpy(count_out, p.count.data(), (size_t)F * sizeof(int32_t));
    std::copy(p.slots.begin(), p.slots.end(), slots_out);
    std::copy(p.live.begin(), p.live.end(), live_out);
    API_END
}

int p3d_debug_video_mean(int device, const float* sum, const int32_t* count, int n, int64_t hw, int offset, float* out) {
    API_BEGIN
    if (!sum || !count || !out) throw P3dError("null argument");
    if (n < 1 || hw < 1 || (int64_t)n * hw > (int64_t)1 << 31) throw P3dError("video_mean: bad shape");
    for (int i = 0; i < n; ++i)
        if (count[i] < 1) throw P3dError("video_mean: frame " + std::to_string(i) + " has count " + std::to_string(count[i]));
    video_hook_device(device, offset);
    const int64_t ne = (int64_t)n * hw;
    Guarded<float> sb((size_t)ne, 8, (size_t)offset, sum), ob((size_t)ne, 8, (size_t)offset, nullptr);
    DevArr<int32_t> cb((size_t)n, count);
    VideoMeanArgs a;
    a.sum = sb.data(); a.count = cb.p; a.out = ob.data(); a.n = n; a.hw = hw;
    if (std::string(p3d_video_mean_desc(a).kernel) != "video_mean_kernel") throw P3dError("video_mean: launch description names another kernel");
    HIPCHECK(p3d_video_mean(a, nullptr));
    HIPCHECK(hipDeviceSynchronize());
    sb.unchanged("video_mean");
    ob.back(out, "video_mean");
    API_END
}

int p3d_debug_video_plan(int mode, int F, int T, int B, int last_start, const int32_t* count_in, const int* starts, int n_windows,
                         int32_t* count_out) {
    API_BEGIN
    if (!count_out) throw P3dError("null argument");
    const p3d_handle::Video::Plan p = p3d_handle::Video::plan(mode, F, T, B, last_start, count_in, nullptr, starts, n_windows);
    memcpy(count_out, p.count.data(), (size_t)F * sizeof(int32_t));
    API_END
}

// ---- temporal smoothing of the video's maps at read-out (include/p3d_hip.h; the handle's part in net_video.inc, temporal.hip) --
int p3d_set_video_temporal(p3d_handle* h, const p3d_video_temporal* cfg) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    h->set_video_temporal(cfg);
    API_END
}

int p3d_get_video_temporal(p3d_handle* h, p3d_video_temporal* cfg, int* on) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    if (cfg) *cfg = h->temporal.cfg.set;
    if (on) *on = h->temporal.cfg.on() ? 1 : 0;
    API_END
}

int p3d_video_temporal_last_ms(p3d_handle* h, double* ms) {
    API_BEGIN
    if (!h || !ms) throw P3dError("null argument");
    if (!h->temporal.timed) throw P3dError("video_temporal_last_ms: no read-out has run the temporal stage");
    HIPCHECK(hipSetDevice(h->cfg.device));
    float t = 0.f;
    HIPCHECK(hipEventElapsedTime(&t, h->temporal.ev[0], h->temporal.ev[1]));
    *ms = (double)t;
    API_END
}

}  // extern "C"
namespace {
// One temporal launch from its launch description on host arrays: store [F][hw], count [F] (null: every count 1) under `mode`,
// frames first .. first + n - 1 -> out [n][hw].  Every refusal is decided before the first HIP call.
void temporal_on_host(int device, int mode, const p3d_video_temporal* cfg, const float* store, const int32_t* count, int F, int64_t hw,
                      int first, int n, int offset, float* out) {
    if (!store || !out) throw P3dError("null argument");
    if (mode != VIDEO_NEWEST && mode != VIDEO_MEAN) throw P3dError("video_temporal: mode " + std::to_string(mode) + " is neither P3D_VIDEO_NEWEST (0) nor P3D_VIDEO_MEAN (1)");
    const p3d_handle::TemporalCfg t = p3d_handle::TemporalCfg::parse(cfg);
    if (!t.on()) throw P3dError("video_temporal: the hook needs a kind (GAUSS or EMA)");
    if (F < 1 || hw < 1 || (int64_t)F * hw > (int64_t)1 << 31) throw P3dError("video_temporal: bad shape");
    std::vector<int32_t> ones;
    if (!count) { ones.assign((size_t)F, 1); count = ones.data(); }
    p3d_handle::TemporalCfg::check("video_temporal", t, F, first, n, count);
    video_hook_device(device, offset);
    const int64_t ns = (int64_t)F * hw, no = (int64_t)n * hw;
    Guarded<float> sb((size_t)ns, 8, (size_t)offset, store), ob((size_t)no, 8, (size_t)offset, nullptr);
    Guarded<int32_t> cb((size_t)F, 8, 0, count);
    const VideoTemporalArgs a = p3d_handle::TemporalCfg::args(t, sb.data(), mode == VIDEO_MEAN ? cb.data() : nullptr, ob.data(), F, hw, first, n);
    const std::string want = std::string(t.set.kind == P3D_TEMPORAL_GAUSS ? "video_temporal_gauss_kernel<" : "video_temporal_ema_kernel<") +
                             (mode == VIDEO_MEAN ? "1>" : "0>");
    if (std::string(p3d_video_temporal_desc(a).kernel) != want) throw P3dError("video_temporal: launch description names another kernel");
    HIPCHECK(p3d_video_temporal_launch(a, nullptr));
    HIPCHECK(hipDeviceSynchronize());
    sb.unchanged("video_temporal");
    cb.unchanged("video_temporal");
    ob.back(out, "video_temporal");
}
}  // namespace
extern "C" {

int p3d_temporal_filter(int device, const p3d_video_temporal* cfg, const float* maps, int F, int64_t hw, int first, int n, float* out) {
    API_BEGIN
    temporal_on_host(device, VIDEO_NEWEST, cfg, maps, nullptr, F, hw, first, n, 0, out);
    API_END
}

int p3d_debug_video_temporal(int device, int mode, const p3d_video_temporal* cfg, const float* store, const int32_t* count, int F,
                             int64_t hw, int first, int n, int offset, float* out) {
    API_BEGIN
    if (!count) throw P3dError("null argument");
    if (offset < 0 || offset > 3) throw P3dError("video hook: offset is 0 .. 3");
    temporal_on_host(device, mode, cfg, store, count, F, hw, first, n, offset, out);
    API_END
}

int p3d_debug_video_temporal_desc(int mode, const p3d_video_temporal* cfg, int F, int64_t hw, int first, int n, char* kernel, int cap,
                                  double* flops, double* bytes) {
    API_BEGIN
    if (!kernel || cap < 1 || !flops || !bytes) throw P3dError("null argument");
    if (mode != VIDEO_NEWEST && mode != VIDEO_MEAN) throw P3dError("video_temporal: mode " + std::to_string(mode) + " is neither P3D_VIDEO_NEWEST (0) nor P3D_VIDEO_MEAN (1)");
    const p3d_handle::TemporalCfg t = p3d_handle::TemporalCfg::parse(cfg);
    if (!t.on()) throw P3dError("video_temporal: the hook needs a kind (GAUSS or EMA)");
    if (F < 1 || hw < 1) throw P3dError("video_temporal: bad shape");
    const std::vector<int32_t> ones((size_t)F, 1);
    p3d_handle::TemporalCfg::check("video_temporal", t, F, first, n, ones.data());
    // (the description reads no memory: the pointers only say which is there)
    const float* some = reinterpret_cast<const float*>(kernel);
    const VideoTemporalArgs a = p3d_handle::TemporalCfg::args(t, some, mode == VIDEO_MEAN ? ones.data() : nullptr, nullptr, F, hw, first, n);
    const LaunchDesc d = p3d_video_temporal_desc(a);
    snprintf(kernel, (size_t)cap, "%s", d.kernel);
    *flops = d.flops; *bytes = d.bytes;
    API_END
}

int p3d_debug_video_temporal_plan(int kind, int r, int64_t hw, int n, int* pixels_per_block, int* frames_per_block, int* lds_bytes) {
    API_BEGIN
    if (!pixels_per_block || !frames_per_block || !lds_bytes) throw P3dError("null argument");
    if (kind != P3D_TEMPORAL_GAUSS && kind != P3D_TEMPORAL_EMA) throw P3dError("video_temporal_plan: the kind is GAUSS (1) or EMA (2)");
    if (kind == P3D_TEMPORAL_GAUSS && (r < 1 || r > P3D_TEMPORAL_MAX_RADIUS))
        throw P3dError("video_temporal_plan: radius must be in [1, " + std::to_string(P3D_TEMPORAL_MAX_RADIUS) + "]");
    if (hw < 1 || n < 1) throw P3dError("video_temporal_plan: at least one pixel and one frame");
    const VideoTemporalPlan p = p3d_video_temporal_plan(kind, r, hw, n);
    *pixels_per_block = p.pixels_per_block; *frames_per_block = p.frames_per_block; *lds_bytes = p.lds_bytes;
    API_END
}

// CRC-32C (Castagnoli) of a host buffer, slicing-by-8: the checksum of TensorFlow's checkpoint bundles
// (tensorflow/core/lib/hash/crc32c.h), used by the Python reader / writer of sap3d_tensorflow_amd/tf_checkpoint.py on the
// 248 MB of variables (train.py:180-185, 204-210, 266-267).  `crc` = running value (0 to start).
uint32_t p3d_crc32c(const void* data, size_t n, uint32_t crc) {
    static uint32_t T[8][256];
    static bool ready = false;
    if (!ready) {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1) ? 0x82F63B78u : 0u);
            T[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; ++i)
            for (int t = 1; t < 8; ++t) T[t][i] = (T[t - 1][i] >> 8) ^ T[0][T[t - 1][i] & 0xFF];
        ready = true;
    }
    const unsigned char* p = (const unsigned char*)data;
    uint32_t c = crc ^ 0xFFFFFFFFu;
    while (n >= 8) {
        uint32_t lo, hi;
        memcpy(&lo, p, 4); memcpy(&hi, p + 4, 4);
        lo ^= c;
        c = T[7][lo & 0xFF] ^ T[6][(lo >> 8) & 0xFF] ^ T[5][(lo >> 16) & 0xFF] ^ T[4][lo >> 24] ^
            T[3][hi & 0xFF] ^ T[2][(hi >> 8) & 0xFF] ^ T[1][(hi >> 16) & 0xFF] ^ T[0][hi >> 24];
        p += 8; n -= 8;
    }
    while (n--) c = T[0][(c ^ *p++) & 0xFF] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

// ---- resident training set (include/p3d_hip.h; the handle's part in net_trainset.inc, the kernel in trainset.hip) ------------------
int p3d_trainset_open(p3d_handle* h, int n_videos, const int* frames, int frame_format, int flags, const float mean_rgb[3]) {
    API_BEGIN
    if (!h || !frames || !mean_rgb) throw P3dError("null argument");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->trainset_open(n_videos, frames, frame_format, flags, mean_rgb);
    API_END
}

int p3d_trainset_close(p3d_handle* h) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->trainset_close();
    API_END
}

int p3d_trainset_info(p3d_handle* h, int* n_videos, int64_t* total_frames, int* frame_format, int* flags, int64_t* bytes) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    h->trainset.need_open("trainset_info");
    if (n_videos) *n_videos = (int)h->trainset.frames.size();
    if (total_frames) *total_frames = h->trainset.total();
    if (frame_format) *frame_format = h->trainset.format;
    if (flags) *flags = h->trainset.flags;
    if (bytes) *bytes = (int64_t)(h->trainset.fr.n + h->trainset.den.n + h->trainset.fix.n);
    API_END
}

int p3d_trainset_video_info(p3d_handle* h, int video, int* frames, int* put_frames, int* put_density, int* put_fixations) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    h->trainset.need_open("trainset_video_info");
    if (video < 0 || video >= (int)h->trainset.frames.size())
        throw P3dError("trainset_video_info: video " + std::to_string(video) + " is outside [0, " + std::to_string(h->trainset.frames.size()) + ")");
    const int F = h->trainset.frames[(size_t)video];
    int* out[3] = {put_frames, put_density, put_fixations};
    for (int t = 0; t < 3; ++t) {
        if (!out[t]) continue;
        const unsigned char* p = h->trainset.put[t].data() + h->trainset.base[(size_t)video];
        *out[t] = (int)std::count(p, p + F, (unsigned char)1);
    }
    if (frames) *frames = F;
    API_END
}

int p3d_trainset_put_frames_u8(p3d_handle* h, int video, int first, const unsigned char* bgr, int n, int H0, int W0) {
    API_BEGIN
    if (!h || !bgr) throw P3dError("null argument");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->trainset_put_frames_u8(video, first, bgr, n, H0, W0);
    API_END
}

int p3d_trainset_put_frames(p3d_handle* h, int video, int first, const float* x, int n) {
    API_BEGIN
    if (!h || !x) throw P3dError("null argument");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->trainset_put_frames(video, first, x, n);
    API_END
}

int p3d_trainset_put_density_u8(p3d_handle* h, int video, int first, const unsigned char* grey, int n, int H0, int W0) {
    API_BEGIN
    if (!h || !grey) throw P3dError("null argument");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->trainset_put_density_u8(video, first, grey, n, H0, W0);
    API_END
}

int p3d_trainset_put_fixations(p3d_handle* h, int video, int first, const unsigned char* fix, int n) {
    API_BEGIN
    if (!h || !fix) throw P3dError("null argument");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->trainset_put_fixations(video, first, fix, n);
    API_END
}

int p3d_trainset_stage(p3d_handle* h, const int* video, const int* start, int n) {
    API_BEGIN
    if (!h || !video || !start) throw P3dError("null argument");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->trainset_gather("trainset_stage", video, start, n, true);
    HIPCHECK(hipStreamSynchronize(h->stream));
    API_END
}

int p3d_trainset_step(p3d_handle* h, const int* video, const int* start, int n, float dropout_rate, uint64_t seed, float* loss) {
    API_BEGIN
    if (!h || !video || !start) throw P3dError("null argument");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->trainset_step_check();
    h->trainset_gather("trainset_step", video, start, n, true);
    h->check_fixations(true);
    h->fix_fresh = false;
    if (h->aug_on) h->augment_staged(seed, nullptr, nullptr);      // p3d_augment_inputs: from the staged buffers themselves
    h->train_step_device(dropout_rate, seed);
    const float l = h->read_loss();
    if (loss) *loss = l;
    API_END
}

int p3d_trainset_forward(p3d_handle* h, const int* video, const int* start, int n, float* pred) {
    API_BEGIN
    if (!h || !video || !start || !pred) throw P3dError("null argument");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->trainset_gather("trainset_forward", video, start, n, false);
    Ctx c; c.training = false; c.drop = 0.f; c.seed = 0; c.update_moving = false; c.s = h->stream;      // p3d_forward's pass
    h->run_forward(c);
    h->download_act(h->pred, pred);
    API_END
}

int p3d_trainset_get_staged(p3d_handle* h, float* x, float* y, unsigned char* fix) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->trainset.need_open("trainset_get_staged");
    if (fix && !h->d_fix) throw P3dError("trainset_get_staged: no fixation maps were ever staged");
    const hipStream_t s = h->stream;
    if (x) HIPCHECK(hipMemcpyAsync(x, h->x_in->p, (size_t)h->x_in->rows() * 3 * sizeof(float), hipMemcpyDeviceToHost, s));
    if (y) HIPCHECK(hipMemcpyAsync(y, h->d_y, (size_t)h->pred->rows() * sizeof(float), hipMemcpyDeviceToHost, s));
    if (fix) HIPCHECK(hipMemcpyAsync(fix, h->d_fix, (size_t)h->pred->rows(), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    API_END
}

int p3d_trainset_last_ms(p3d_handle* h, double* ms) {
    API_BEGIN
    if (!h || !ms) throw P3dError("null argument");
    h->trainset.need_open("trainset_last_ms");
    if (!h->trainset.timed) throw P3dError("trainset_last_ms: nothing was staged from the open training set");
    HIPCHECK(hipSetDevice(h->cfg.device));
    float t = 0.f;
    HIPCHECK(hipEventElapsedTime(&t, h->trainset.ev[0], h->trainset.ev[1]));
    *ms = (double)t;
    API_END
}

// The launch of trainset.hip from its launch description, on host arrays.  Every device buffer sits `offset` elements past a 16-byte
// boundary between guard elements; a guard or a store that the launch changed is an error.
int p3d_debug_trainset_gather(int device, int frame_format, const void* frames_store, const unsigned char* density_store,
                              const unsigned char* fix_store, int n_videos, const int* frames, int T, int64_t hw, const float mean_rgb[3],
                              const int* video, const int* start, const int* first, int B, int offset, float* x, float* y,
                              unsigned char* fix) {
    API_BEGIN
    if (!frames_store || !frames || !mean_rgb || !video || !start || !x) throw P3dError("null argument");
    if ((y != nullptr) != (density_store != nullptr) || (fix != nullptr) != (fix_store != nullptr))
        throw P3dError("trainset_gather: a store and its output come together");
    if (frame_format != P3D_TRAINSET_FRAMES_U8 && frame_format != P3D_TRAINSET_FRAMES_F32) throw P3dError("trainset_gather: unknown frame format");
    if (n_videos < 1 || T < 1 || hw < 1 || B < 1) throw P3dError("trainset_gather: bad shape");
    int64_t total = 0;
    std::vector<int64_t> base((size_t)n_videos, 0);
    for (int v = 0; v < n_videos; ++v) {
        if (frames[v] < 1) throw P3dError("trainset_gather: a video without frames");
        base[(size_t)v] = total;
        total += frames[v];
    }
    if (total * hw * 3 > (int64_t)1 << 28 || (int64_t)B * T * hw * 3 > (int64_t)1 << 28) throw P3dError("trainset_gather: the hook takes up to 2^28 elements");
    video_hook_device(device, offset);
    std::vector<int> fr((size_t)B, 0);      // a row the wrapper will refuse keeps 0 here: it is never dereferenced
    for (int k = 0; k < B; ++k)
        fr[(size_t)k] = first ? first[k] : (video[k] >= 0 && video[k] < n_videos ? (int)(base[(size_t)video[k]] + start[k]) : 0);
    const bool f32 = frame_format == P3D_TRAINSET_FRAMES_F32;
    const int64_t npx = total * hw, nout = (int64_t)B * T * hw;
    const size_t off = (size_t)offset;
    Guarded<float> sf(f32 ? (size_t)npx * 3 : 0, 16, off, f32 ? (const float*)frames_store : nullptr), xb((size_t)nout * 3, 16, off, nullptr),
        yb(y ? (size_t)nout : 0, 16, off, nullptr);
    Guarded<unsigned char> su(f32 ? 0 : (size_t)npx * 3, 16, off, f32 ? nullptr : (const unsigned char*)frames_store),
        sd(y ? (size_t)npx : 0, 16, off, density_store), sx(fix ? (size_t)npx : 0, 16, off, fix_store), fb(fix ? (size_t)nout : 0, 16, off, nullptr);
    DevArr<int> tab((size_t)B, fr.data());
    TrainsetGatherArgs a;
    a.format = f32 ? TRAINSET_F32 : TRAINSET_U8;
    a.frames = f32 ? (const void*)sf.data() : (const void*)su.data();
    a.density = y ? sd.data() : nullptr; a.fixations = fix ? sx.data() : nullptr;
    a.x = xb.data(); a.y = y ? yb.data() : nullptr; a.fix = fix ? fb.data() : nullptr;
    a.first = tab.p; a.first_host = fr.data(); a.video_host = video; a.start_host = start; a.frames_host = frames; a.n_videos = n_videos;
    a.B = B; a.T = T; a.hw = hw;
    for (int c = 0; c < 3; ++c) a.mean[c] = mean_rgb[c];
    if (std::string(p3d_trainset_gather_desc(a).kernel) != "trainset_gather_kernel<" + std::to_string(a.format) + ">")
        throw P3dError("trainset_gather: launch description names another kernel");
    HIPCHECK(p3d_trainset_gather(a, nullptr));
    HIPCHECK(hipDeviceSynchronize());
    sf.unchanged("trainset_gather"); su.unchanged("trainset_gather"); sd.unchanged("trainset_gather"); sx.unchanged("trainset_gather");
    xb.back(x, "trainset_gather");
    yb.back(y, "trainset_gather");
    fb.back(fix, "trainset_gather");
    API_END
}

}  // extern "C"
