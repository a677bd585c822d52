// part of net.hip: the C ABI of include/p3d_hip.h over p3d_handle (one entry point per reference interface, cited there), the
// single-operator entry points of the op-level parity tests, and the test hooks (p3d_debug_*).
// ==================================================================================================
#define API_BEGIN try {
#define API_END                                        \
    }                                                  \
    catch (const std::exception& e) {                  \
        g_err = e.what();                              \
        return -1;                                     \
    }                                                  \
    return 0;

extern "C" {

const char* p3d_last_error(void) { return g_err.c_str(); }

void p3d_default_config(p3d_config* c) {
    memset(c, 0, sizeof(*c));
    c->structure = P3D_STRUCTURE_UNET;
    c->batch = 2; c->frames = 16; c->height = 112; c->width = 112; c->base = 64;
    c->blocks[0] = 3; c->blocks[1] = 8; c->blocks[2] = 36;
    c->device = 0; c->world_size = 1; c->rank = 0;
}

// Two HIP runtimes in one process (e.g. /opt/rocm's, which this library links, next to the copy a PyTorch wheel bundles)
// end in heap corruption at exit.  Callers that bind the library by hand get the diagnosis here instead of there.
static void refuse_two_hip_runtimes() {
    FILE* f = fopen("/proc/self/maps", "r");
    if (!f) return;
    std::vector<std::string> seen;
    char line[1024];
    while (fgets(line, sizeof(line), f)) {
        const char* p = strstr(line, "libamdhip64.so");
        if (!p) continue;
        const char* path = strchr(line, '/');
        if (!path) continue;
        std::string s(path);
        while (!s.empty() && (s.back() == '\n' || s.back() == ' ')) s.pop_back();
        if (std::find(seen.begin(), seen.end(), s) == seen.end()) seen.push_back(s);
    }
    fclose(f);
    if (seen.size() > 1)
        throw P3dError("two HIP runtimes are mapped into this process (" + seen[0] + " and " + seen[1] +
                       "): load the one PyTorch bundles before libp3dhip.so (INTEGRATION.md, 'One HIP runtime per process')");
}

// Test hook: a C-level backtrace on SIGABRT / SIGSEGV (glibc backtrace_symbols_fd: async-signal-safe enough for a dying process) and
// the message of an uncaught C++ exception.  Python's faulthandler shows the Python frames only; an abort inside the HIP runtime or in
// this library's host code shows here.  tests/conftest.py installs it once per test process.
#include <execinfo.h>
#include <signal.h>
#include <unistd.h>
#include <exception>
namespace {
void abort_trace_handler(int sig) {
    static const char msg[] = "\n[p3d] fatal signal; C backtrace:\n";
    (void)!write(2, msg, sizeof(msg) - 1);
    void* frames[64];
    const int n = backtrace(frames, 64);
    backtrace_symbols_fd(frames, n, 2);
    signal(sig, SIG_DFL);
    raise(sig);
}
void terminate_trace() {
    if (std::exception_ptr e = std::current_exception()) {
        try { std::rethrow_exception(e); }
        catch (const std::exception& ex) { fprintf(stderr, "[p3d] std::terminate: uncaught exception: %s\n", ex.what()); }
        catch (...) { fprintf(stderr, "[p3d] std::terminate: uncaught non-standard exception\n"); }
    } else fprintf(stderr, "[p3d] std::terminate without an active exception\n");
    fflush(stderr);
    abort();
}
}  // namespace
int p3d_debug_install_abort_trace(void) {
    signal(SIGABRT, abort_trace_handler);
    signal(SIGSEGV, abort_trace_handler);
    std::set_terminate(terminate_trace);
    return 0;
}

int p3d_create(const p3d_config* cfg, p3d_handle** out) {
    p3d_handle* h = nullptr;
    try {
        if (!cfg || !out) throw P3dError("null argument");
        refuse_two_hip_runtimes();
        int ndev = 0;
        HIPCHECK(hipGetDeviceCount(&ndev));
        if (ndev <= 0) throw P3dError("no HIP device: libp3dhip has no CPU fallback");
        if (cfg->device < 0 || cfg->device >= ndev) throw P3dError("bad device ordinal");
        HIPCHECK(hipSetDevice(cfg->device));
        h = new p3d_handle();
        h->cfg = *cfg;
        if (const long mb = bucket_mb_env(); mb >= 1) h->bucket_floats = (int64_t)mb * (1 << 18);
        if (const char* e = p3d_tune_env("P3D_FUSE_MAX_ROWS")) h->fuse_max_rows = atoll(e);      // A/B runs: which bottlenecks are built fusable
        ensure_zero_page();
        {   // the main stream carries the dependent chain of small launches and the comm stream the all-reduces: both above
            // the side stream's filter gradients (measured: no effect on the step time on this ROCm, 17.98 vs 17.95 ms;
            // what does help is keeping the filter gradients' residency low, conv_wgrad2.hip launch_group_t)
            h->stream = take_stream(cfg->device, 0);
            if (const char* e = p3d_tune_env("P3D_MAIN_CU_MASK")) {      // experiment (tuning build): the main stream on a CU subset (l128 / h128: the lower / upper 128 mask bits).
                // Only CONTIGUOUS masks take effect on ROCm 7.2: strided ones (every 2nd / 8th bit) change nothing (round 5) -- which voids round 4's "reserving every 8th CU" run
                uint32_t mask[8];
                for (int w = 0; w < 8; ++w) mask[w] = 0xffffffffu;
                const int v = atoi(e + 1);
                if (e[0] == 'l') { for (int b = v; b < 256; ++b) mask[b >> 5] &= ~(1u << (b & 31)); }
                else if (e[0] == 'h') { for (int b = 0; b < v; ++b) mask[b >> 5] &= ~(1u << (b & 31)); }                   // h128: the upper 128 bits
                else if (e[0] == 's' && v > 1) { for (int b = v - 1; b < 256; b += v) mask[b >> 5] &= ~(1u << (b & 31)); }
                else if (e[0] == 'o' && v > 1) { for (int b = 0; b < 256; ++b) if ((b % v) != v - 1) mask[b >> 5] &= ~(1u << (b & 31)); }
                give_stream(cfg->device, 0, h->stream);
                HIPCHECK(hipExtStreamCreateWithCUMask(&h->stream, 8, mask));      // (leaked into the pool at destroy: a diagnostic process)
            }
            h->comm_stream = take_stream(cfg->device, 0);
            if (const char* e = p3d_tune_env("P3D_SIDE_CU_MASK")) {      // experiment: keep some CUs free of the side stream's filter gradients
                uint32_t mask[8];
                for (int w = 0; w < 8; ++w) mask[w] = 0xffffffffu;
                const int v = atoi(e + 1);
                if (e[0] == 'l') { for (int b = v; b < 256; ++b) mask[b >> 5] &= ~(1u << (b & 31)); }            // l224: the lowest 224 bits
                else if (e[0] == 'h') { for (int b = 0; b < v; ++b) mask[b >> 5] &= ~(1u << (b & 31)); }
                else if (e[0] == 's' && v > 1) { for (int b = v - 1; b < 256; b += v) mask[b >> 5] &= ~(1u << (b & 31)); }   // s8: every 8th bit off
                else if (e[0] == 'o' && v > 1) { for (int b = 0; b < 256; ++b) if ((b % v) != v - 1) mask[b >> 5] &= ~(1u << (b & 31)); }   // o2: only every 2nd bit on
                HIPCHECK(hipExtStreamCreateWithCUMask(&h->side_stream, 8, mask));
                h->side_pooled = false;
            } else
            h->side_stream = take_stream(cfg->device, 1);
        }
        HIPCHECK(hipEventCreateWithFlags(&h->ev_side_done, hipEventDisableTiming));
        HIPCHECK(hipEventCreateWithFlags(&h->ev_side_early, hipEventDisableTiming));
        HIPCHECK(hipEventCreateWithFlags(&h->ev_comm_early, hipEventDisableTiming));
        HIPCHECK(hipEventCreateWithFlags(&h->ev_side_bucket, hipEventDisableTiming));
        HIPCHECK(hipEventCreateWithFlags(&h->ev_bucket, hipEventDisableTiming));
        HIPCHECK(hipEventCreateWithFlags(&h->ev_comm_done, hipEventDisableTiming));
        if (cfg->structure < P3D_STRUCTURE_UNET || cfg->structure > P3D_STRUCTURE_UNETPP_DS) throw P3dError("unknown structure");
        if (cfg->batch < 1) throw P3dError("batch must be >= 1");
        for (int i = 0; i < 3; ++i)
            if (cfg->blocks[i] < 1) throw P3dError("blocks must be >= 1");
        if (cfg->structure == P3D_STRUCTURE_CONCAT) h->build_concat();
        else if (cfg->structure == P3D_STRUCTURE_GN_P3D) h->build_gn_p3d(16);
        else if (cfg->structure == P3D_STRUCTURE_GN_P3D_CONCAT) h->build_gn_p3d(8);
        else if (cfg->structure == P3D_STRUCTURE_UNETPP_NONSA) h->build_unetpp(false);
        else if (cfg->structure == P3D_STRUCTURE_UNETPP_DS) h->build_unetpp(true);
        else if (cfg->structure == P3D_STRUCTURE_GN_P3D_DECODER) h->build_gn_decoder();
        else h->build_unet();
        h->finalize_build();
        HIPCHECK(hipStreamSynchronize(h->stream));
        *out = h;
        ++g_live_handles;
    } catch (const std::exception& e) {
        g_err = e.what();
        hipDeviceSynchronize();      // the handle's streams go back to the pool: nothing of the failed build may still be queued on them
        delete h;
        return -1;
    }
    return 0;
}

void p3d_destroy(p3d_handle* h) {
    if (!h) return;
    hipSetDevice(h->cfg.device);
    hipDeviceSynchronize();
    if (g_perturb == &h->perturb) g_perturb = nullptr;
    delete h;
    --g_live_handles;
}

int p3d_num_params(p3d_handle* h) { return h ? (int)h->porder.size() : -1; }

int p3d_param_info(p3d_handle* h, int index, const char** name, int* ndim, int64_t shape[5], int* trainable) {
    API_BEGIN
    if (!h || index < 0 || index >= (int)h->porder.size()) throw P3dError("bad parameter index");
    Param* p = h->porder[index];
    if (name) *name = p->name.c_str();
    if (ndim) *ndim = (int)p->shape.size();
    if (shape)
        for (size_t i = 0; i < 5; ++i) shape[i] = i < p->shape.size() ? p->shape[i] : 1;
    if (trainable) *trainable = p->trainable;
    API_END
}

static Param* find_param(p3d_handle* h, const char* name, int64_t count) {
    if (!h || !name) throw P3dError("null argument");
    auto it = h->pindex.find(name);
    if (it == h->pindex.end()) throw P3dError(std::string("no variable named ") + name);
    if (count != it->second->count)
        throw P3dError(std::string("size mismatch for ") + name + ": got " + std::to_string(count) + ", variable has " +
                       std::to_string(it->second->count));
    return it->second;
}

int p3d_set_param(p3d_handle* h, const char* name, const float* host, int64_t count) {
    API_BEGIN
    Param* p = find_param(h, name, count);
    h->refuse_swapped("p3d_set_param");
    HIPCHECK(hipSetDevice(h->cfg.device));
    // the handle's streams are non-blocking: nothing else orders this copy after a step that is still running
    HIPCHECK(hipStreamSynchronize(h->stream));
    HIPCHECK(hipStreamSynchronize(h->side_stream));
    HIPCHECK(hipStreamSynchronize(h->comm_stream));
    HIPCHECK(copy_now(p->p, host, (size_t)count * 4, hipMemcpyHostToDevice, h->stream));
    API_END
}
int p3d_get_param(p3d_handle* h, const char* name, float* host, int64_t count) {
    API_BEGIN
    Param* p = find_param(h, name, count);
    HIPCHECK(hipSetDevice(h->cfg.device));
    HIPCHECK(copy_now(host, p->p, (size_t)count * 4, hipMemcpyDeviceToHost, h->stream));
    API_END
}
int p3d_get_grad(p3d_handle* h, const char* name, float* host, int64_t count) {
    API_BEGIN
    Param* p = find_param(h, name, count);
    if (!p->trainable) throw P3dError(std::string(name) + " is not trainable");
    HIPCHECK(hipSetDevice(h->cfg.device));
    HIPCHECK(copy_now(host, p->g, (size_t)count * 4, hipMemcpyDeviceToHost, h->stream));
    API_END
}

int p3d_init_params(p3d_handle* h, uint64_t seed) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    h->refuse_swapped("p3d_init_params");
    HIPCHECK(hipSetDevice(h->cfg.device));
    uint64_t idx = 0;
    for (Param* p : h->porder) {
        ++idx;
        if (p->init == INIT_XAVIER) {
            // tf.contrib.layers.xavier_initializer: U(-L, L), L = sqrt(6 / (fan_in + fan_out)); rank-1 [C]: fans = C
            double fi, fo;
            if (p->shape.size() == 1) fi = fo = (double)p->shape[0];
            else {
                double rf = 1;
                for (size_t i = 0; i + 2 < p->shape.size(); ++i) rf *= (double)p->shape[i];
                fi = rf * p->shape[p->shape.size() - 2];
                fo = rf * p->shape[p->shape.size() - 1];
            }
            const float L = (float)std::sqrt(6.0 / (fi + fo));
            HIPCHECK(p3d_fill_uniform(p->p, p->count, -L, L, seed * 0x9E3779B97F4A7C15ull + idx, h->stream));
        } else if (p->init == INIT_VS) {
            // tf.contrib.layers.variance_scaling_initializer() defaults (utils/network.py:212-213,264): factor 2.0,
            // mode FAN_IN, uniform False -> truncated normal with stddev sqrt(1.3 * 2 / fan_in) (the 1.3 is TF's
            // correction for the variance the truncation at two standard deviations removes)
            double rf = 1;
            for (size_t i = 0; i + 2 < p->shape.size(); ++i) rf *= (double)p->shape[i];
            const double fan_in = rf * p->shape[p->shape.size() - 2];
            HIPCHECK(p3d_fill_trunc_normal(p->p, p->count, (float)std::sqrt(1.3 * 2.0 / fan_in), seed * 0x9E3779B97F4A7C15ull + idx, h->stream));
        } else {
            const float v = p->init == INIT_ONES ? 1.f : 0.f;
            HIPCHECK(p3d_fill_uniform(p->p, p->count, v, v, 0, h->stream));
        }
    }
    HIPCHECK(hipMemsetAsync(h->flat_m, 0, (size_t)h->n_train * 4, h->stream));
    HIPCHECK(hipMemsetAsync(h->flat_v, 0, (size_t)h->n_train * 4, h->stream));
    h->step = 0;
    HIPCHECK(hipStreamSynchronize(h->stream));
    if (h->ema_on) h->ema_seed();      // fresh variables, fresh shadows
    h->acc_pending = 0;                // and no partial sum of gradients (p3d_set_grad_accum)
    API_END
}

int p3d_upload_inputs(p3d_handle* h, const float* x, const float* y) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->upload(x, y);
    HIPCHECK(hipStreamSynchronize(h->stream));
    API_END
}

int p3d_forward_device(p3d_handle* h, int training, float dropout_rate, uint64_t seed) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    HIPCHECK(hipSetDevice(h->cfg.device));
    Ctx c; c.training = training != 0; c.drop = dropout_rate; c.seed = seed; c.update_moving = false; c.s = h->stream;
    h->run_forward(c);
    API_END
}

int p3d_forward(p3d_handle* h, const float* x, int training, float dropout_rate, uint64_t seed, float* pred) {
    API_BEGIN
    if (!h || !x || !pred) throw P3dError("null argument");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->upload(x, nullptr);
    Ctx c; c.training = training != 0; c.drop = dropout_rate; c.seed = seed; c.update_moving = false; c.s = h->stream;
    h->run_forward(c);
    h->download_act(h->pred, pred);
    API_END
}

int p3d_set_pointwise_fp16(p3d_handle* h, int enable) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    h->pointwise_f16 = enable != 0;
    API_END
}

int64_t p3d_debug_dirty_counters(void) { return (int64_t)p3d_scratch_dirty_counters(); }

int p3d_debug_force_plan(int igemm_tile, int igemm_splits, int wgrad_tm, int wgrad_tn) {
    p3d_igemm2_override(igemm_tile, igemm_splits);
    p3d_wgrad2_force_tile(wgrad_tm, wgrad_tn);
    return 0;
}

int p3d_set_attention_mode(p3d_handle* h, int mode) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    if (mode < 0 || mode > 2) throw P3dError("attention mode is 0 (per site), 1 (stored scores) or 2 (flash)");
    HIPCHECK(hipSetDevice(h->cfg.device));
    if (mode == 1) for (auto& f : h->attn_gemm_alloc) f();      // sites that were built flash-only get their score buffers now
    h->attn_mode = mode;
    h->drop_step_graph();
    API_END
}

int p3d_set_loss(p3d_handle* h, int kind) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    if (kind != P3D_LOSS_SMOOTH_L1 && kind != P3D_LOSS_BCE && kind != P3D_LOSS_L1 && kind != P3D_LOSS_KLD_CC && kind != P3D_LOSS_SALIENCY)
        throw P3dError("loss kind is 0 (Smooth-L1), 1 (sigmoid cross-entropy on the logits), 2 (L1 sum), 3 (per-map KL + CC) or "
                       "4 (per-map KL + CC + NSS + SIM), not " + std::to_string(kind));
    HIPCHECK(hipSetDevice(h->cfg.device));
    if (kind == P3D_LOSS_SALIENCY && !h->d_sal_scratch) {      // planned once, here: a step allocates nothing
        size_t md = 0, mc = 0;
        p3d_saliency_loss_scratch((long long)h->pred->N * h->pred->D, (long long)h->pred->H * h->pred->W, &md, &mc);
        h->d_sal_scratch = h->dalloc<double>((int64_t)md);
        h->d_sal_cnt = h->dalloc<unsigned>((int64_t)mc);
        HIPCHECK(fill_now(h->d_sal_cnt, 0, mc * sizeof(unsigned), h->stream));
    }
    h->loss_kind = kind;
    h->drop_step_graph();      // a captured step names the loss kernel it was captured with
    API_END
}

int p3d_set_loss_weights(p3d_handle* h, float kld_weight, float cc_weight) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    if (!std::isfinite(kld_weight) || !std::isfinite(cc_weight) || kld_weight < 0.f || cc_weight < 0.f)
        throw P3dError("loss weights must be finite and not negative");
    if (kld_weight == 0.f && cc_weight == 0.f) throw P3dError("loss weights: both are 0");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->kld_weight = kld_weight;
    h->cc_weight = cc_weight;
    h->drop_step_graph();      // the weights are launch arguments of the captured loss launches
    API_END
}

int p3d_set_saliency_weights(p3d_handle* h, float kld, float cc, float nss, float sim) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    for (float w : {kld, cc, nss, sim})
        if (!std::isfinite(w) || w < 0.f) throw P3dError("saliency loss weights must be finite and not negative");
    if (kld == 0.f && cc == 0.f && nss == 0.f && sim == 0.f) throw P3dError("saliency loss weights: all four are 0");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->sal_kld = kld; h->sal_cc = cc; h->sal_nss = nss; h->sal_sim = sim;
    h->drop_step_graph();      // the weights are launch arguments of the captured loss launches
    API_END
}

int p3d_upload_fixations(p3d_handle* h, const unsigned char* fix) {
    API_BEGIN
    if (!h || !fix) throw P3dError("null argument");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->upload_fixations(fix);
    HIPCHECK(hipStreamSynchronize(h->stream));
    API_END
}

int p3d_last_loss_terms(p3d_handle* h, double sums[4], int64_t counts[4]) {
    API_BEGIN
    if (!h || !sums || !counts) throw P3dError("null argument");
    if (h->last_loss_kind != P3D_LOSS_SALIENCY)
        throw P3dError("loss terms: the last step or backward did not run P3D_LOSS_SALIENCY (p3d_set_loss kind 4)");
    HIPCHECK(hipSetDevice(h->cfg.device));
    const size_t maps = (size_t)h->pred->N * h->pred->D;
    std::vector<double> st(maps * (P3D_MAP_STATS + P3D_SAL_STATS));
    HIPCHECK(hipMemcpyAsync(st.data(), h->d_sal_scratch, st.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    const double* ms = st.data();
    const double* xs = st.data() + maps * P3D_MAP_STATS;
    for (int k = 0; k < 4; ++k) { sums[k] = 0.0; counts[k] = 0; }
    for (size_t m = 0; m < maps; ++m) {      // in map order; a term that is undefined on a map (NaN) is left out of its sum and count
        const double v[4] = {ms[m * P3D_MAP_STATS + 2], ms[m * P3D_MAP_STATS + 3], xs[m * P3D_SAL_STATS + 6], xs[m * P3D_SAL_STATS + 7]};
        for (int k = 0; k < 4; ++k)
            if (!std::isnan(v[k])) { sums[k] += v[k]; ++counts[k]; }
    }
    API_END
}

int p3d_set_regularization(p3d_handle* h, int terms, float wd, float l2) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->set_regularization(terms, wd, l2);
    API_END
}

int p3d_last_regularization(p3d_handle* h, double* term) {
    API_BEGIN
    if (!h || !term) throw P3dError("null argument");
    HIPCHECK(hipSetDevice(h->cfg.device));
    *term = h->read_regularization();
    API_END
}

int p3d_param_regularization(p3d_handle* h, const char* name, float* c_wd, float* c_l2) {
    API_BEGIN
    if (!h || !name || !c_wd || !c_l2) throw P3dError("null argument");
    auto it = h->pindex.find(name);
    if (it == h->pindex.end()) throw P3dError(std::string("no variable ") + name);
    if (!it->second->trainable) throw P3dError(std::string(name) + " is not trainable");
    *c_wd = (float)h->reg_coef64(it->second, P3D_REG_WEIGHT_DECAY);
    *c_l2 = (float)h->reg_coef64(it->second, P3D_REG_L2);
    API_END
}

int p3d_set_grad_clip(p3d_handle* h, float clip_norm) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->set_grad_clip(clip_norm);
    API_END
}

int p3d_get_grad_norm(p3d_handle* h, double* sumsq, double* norm, float* scale) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->read_grad_norm(sumsq, norm, scale);
    API_END
}

int p3d_set_grad_accum(p3d_handle* h, int k) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->set_grad_accum(k);
    API_END
}

int p3d_get_grad_accum(p3d_handle* h, int* k, int* pending) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    if (k) *k = h->acc_k;
    if (pending) *pending = h->acc_pending;
    API_END
}

int p3d_set_ema(p3d_handle* h, double decay, int warmup) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->set_ema(decay, warmup != 0);
    API_END
}

int p3d_get_ema(p3d_handle* h, const char* var, float* host, int64_t count) {
    API_BEGIN
    if (!h || !host) throw P3dError("null argument");
    float* d = h->ema_ptr(var, count);
    HIPCHECK(hipSetDevice(h->cfg.device));
    HIPCHECK(copy_now(host, d, (size_t)count * 4, hipMemcpyDeviceToHost, h->stream));
    API_END
}

int p3d_set_ema_var(p3d_handle* h, const char* var, const float* host, int64_t count) {
    API_BEGIN
    if (!h || !host) throw P3dError("null argument");
    float* d = h->ema_ptr(var, count);
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->sync_streams();      // as p3d_set_param: nothing else orders this copy after a running step
    HIPCHECK(copy_now(d, host, (size_t)count * 4, hipMemcpyHostToDevice, h->stream));
    API_END
}

int p3d_ema_swap(p3d_handle* h) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->ema_swap();
    API_END
}

int p3d_ema_swapped(p3d_handle* h) { return h ? (h->ema_swapped ? 1 : 0) : -1; }

int p3d_set_bn_fusion(p3d_handle* h, int enable) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    h->fuse_bn = enable != 0;
    h->fuse_bn_bwd = enable >= 2;
    h->drop_step_graph();
    API_END
}

int p3d_predict_windows(p3d_handle* h, const float* x, float* pred) {
    API_BEGIN
    if (!h || !x || !pred) throw P3dError("null argument");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->upload(x, nullptr);
    Ctx c; c.training = false; c.drop = 0.f; c.update_moving = false; c.per_sample = true; c.s = h->stream;
    h->run_forward(c);
    h->download_act(h->pred, pred);
    API_END
}

int p3d_backward(p3d_handle* h, const float* x, const float* y, float dropout_rate, uint64_t seed, float* loss, float* pred) {
    API_BEGIN
    if (!h || !x || !y) throw P3dError("null argument");
    h->refuse_swapped("p3d_backward");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->check_fixations(true);
    h->fix_fresh = false;
    h->upload(x, y);
    Ctx c; c.training = true; c.drop = dropout_rate; c.seed = seed; c.update_moving = false; c.s = h->stream;
    h->run_forward(c);
    h->run_loss(c);
    h->run_backward(c, false);
    if (h->clip_on()) h->sumsq_range(c, 0, h->n_train);            // the norm of g + c w, before g is rewritten to it; nothing is scaled
    if (h->reg_terms) h->adam_range(c, 0, h->n_train, false);      // the regularisation's gradient, after the backward's
    const float l = h->read_loss();
    if (loss) *loss = l;
    if (pred) h->download_act(h->pred, pred);
    API_END
}

int p3d_train_step_device(p3d_handle* h, float dropout_rate, uint64_t seed) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->train_step_device(dropout_rate, seed);
    API_END
}

int p3d_debug_schedule(p3d_handle* h, float dropout_rate, uint64_t seed, char* text, int64_t cap, int64_t* needed) {
    API_BEGIN
    if (!h || !needed) throw P3dError("null argument");
    HIPCHECK(hipSetDevice(h->cfg.device));
    if (h->graphs_enabled()) throw P3dError("the schedule trace follows the eager launch list (P3D_GRAPH is set)");
    SchedTrace tr;
    tr.streams[h->stream] = "main";
    if (h->side_stream) tr.streams[h->side_stream] = "side";
    if (h->comm_stream) tr.streams[h->comm_stream] = "comm";
    g_trace = &tr;
    try {
        h->train_step_device(dropout_rate, seed);
    } catch (...) {
        g_trace = nullptr;
        throw;
    }
    g_trace = nullptr;
    HIPCHECK(hipStreamSynchronize(h->stream));
    std::string out;
    for (const std::string& l : tr.lines) { out += l; out += '\n'; }
    *needed = (int64_t)out.size() + 1;
    if (text && cap >= *needed) memcpy(text, out.c_str(), out.size() + 1);
    API_END
}

int p3d_debug_perturb(p3d_handle* h, int mode, int stream, int delay_us) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    if (mode < 0 || mode > 2) throw P3dError("perturb: mode is 0 (off), 1 (serial) or 2 (slow)");
    if (mode == 2 && (stream < 0 || stream > 2)) throw P3dError("perturb: stream is 0 (main), 1 (side) or 2 (comm)");
    if (mode == 2 && (delay_us < 1 || delay_us > 2000)) throw P3dError("perturb: delay_us must be in [1, 2000]");
    if (h->graphs_enabled()) throw P3dError("the perturbation follows the eager launch list (P3D_GRAPH is set)");
    Perturb& p = h->perturb;
    p = Perturb();
    p.mode = mode;
    p.streams[0] = h->stream; p.streams[1] = h->side_stream; p.streams[2] = h->comm_stream;
    if (mode == 2) { p.target = p.streams[stream]; p.delay_us = delay_us; }
    if (mode) g_perturb = &p;
    else if (g_perturb == &p) g_perturb = nullptr;
    API_END
}

int p3d_debug_perturb_count(p3d_handle* h, int64_t* delays, int64_t* syncs) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    if (delays) *delays = h->perturb.delays;
    if (syncs) *syncs = h->perturb.syncs;
    API_END
}

int p3d_debug_private_resources(int64_t* blocks, int64_t* bytes, int64_t* events) {
    API_BEGIN
    if (blocks) *blocks = g_dev_blocks.load();
    if (bytes) *bytes = g_dev_bytes.load();
    if (events) *events = g_dev_events.load();
    API_END
}

int p3d_train_step(p3d_handle* h, const float* x, const float* y, float dropout_rate, uint64_t seed, float* loss) {
    API_BEGIN
    if (!h || !x || !y) throw P3dError("null argument");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->refuse_swapped("train step");
    h->check_fixations(true);
    h->fix_fresh = false;
    if (h->aug_on) h->augment_staged(seed, x, y);      // p3d_set_augment: x and y reach the staged buffers through the transform
    else h->upload(x, y);
    h->train_step_device(dropout_rate, seed);
    const float l = h->read_loss();
    if (loss) *loss = l;
    API_END
}

int p3d_set_augment(p3d_handle* h, const p3d_augment* cfg) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->set_augment(cfg);
    API_END
}

int p3d_get_augment(p3d_handle* h, p3d_augment* cfg, int* on) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    if (cfg) *cfg = h->aug_cfg;
    if (on) *on = h->aug_on ? 1 : 0;
    API_END
}

int p3d_augment_inputs(p3d_handle* h, uint64_t seed) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    HIPCHECK(hipSetDevice(h->cfg.device));
    h->augment_staged(seed, nullptr, nullptr);
    HIPCHECK(hipStreamSynchronize(h->stream));
    API_END
}

int p3d_last_augment(p3d_handle* h, int32_t* geom, float* photo) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    if (!h->aug_on) throw P3dError("augmentation: the option is off (p3d_set_augment)");
    if (!h->aug_have) throw P3dError("augmentation: nothing was augmented since the option was switched on");
    for (size_t b = 0; b < h->aug_tab.size(); ++b) {
        const P3dAugClip& k = h->aug_tab[b];
        if (geom) { int32_t* g = geom + 6 * b; g[0] = k.flip; g[1] = k.reverse; g[2] = k.y0; g[3] = k.x0; g[4] = k.ch; g[5] = k.cw; }
        if (photo) { photo[2 * b] = k.a; photo[2 * b + 1] = k.b; }
    }
    API_END
}

int p3d_last_augment_ms(p3d_handle* h, double* ms) {
    API_BEGIN
    if (!h || !ms) throw P3dError("null argument");
    if (!h->aug_on || !h->aug_have) throw P3dError("augmentation: nothing was augmented (p3d_set_augment)");
    HIPCHECK(hipSetDevice(h->cfg.device));
    HIPCHECK(hipEventSynchronize(h->aug_ev[1]));
    float t = 0.f;
    HIPCHECK(hipEventElapsedTime(&t, h->aug_ev[0], h->aug_ev[1]));
    *ms = (double)t;
    API_END
}

int p3d_debug_augment_draw(uint64_t seed, uint64_t g, int H, int W, const p3d_augment* cfg, int32_t geom[6], float photo[2]) {
    API_BEGIN
    if (!cfg || !geom || !photo) throw P3dError("null argument");
    if (H < 1 || W < 1 || !p3d_handle::aug_cfg_valid(*cfg)) throw P3dError("augment_draw: bad grid or configuration");
    const P3dAugClip k = p3d_handle::aug_draw(seed, g, H, W, *cfg);
    geom[0] = k.flip; geom[1] = k.reverse; geom[2] = k.y0; geom[3] = k.x0; geom[4] = k.ch; geom[5] = k.cw;
    photo[0] = k.a; photo[1] = k.b;
    API_END
}

int p3d_last_loss(p3d_handle* h, float* loss) {
    API_BEGIN
    if (!h || !loss) throw P3dError("null argument");
    HIPCHECK(hipSetDevice(h->cfg.device));
    *loss = h->read_loss();
    API_END
}

int p3d_synchronize(p3d_handle* h) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    HIPCHECK(hipSetDevice(h->cfg.device));
    HIPCHECK(hipStreamSynchronize(h->stream));
    HIPCHECK(hipStreamSynchronize(h->side_stream));
    HIPCHECK(hipStreamSynchronize(h->comm_stream));
    API_END
}

int p3d_set_adam(p3d_handle* h, float lr, float beta1, float beta2, float eps) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    h->lr = lr; h->b1 = beta1; h->b2 = beta2; h->eps = eps;
    API_END
}

int p3d_set_optimizer(p3d_handle* h, int kind, float lr, float momentum, int use_nesterov) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    if (kind != P3D_OPT_ADAM && kind != P3D_OPT_MOMENTUM && kind != P3D_OPT_SGD)
        throw P3dError("optimizer kind " + std::to_string(kind) + ": have 0 (adam), 1 (momentum), 2 (sgd)");
    if (!std::isfinite(lr) || !std::isfinite(momentum) || momentum < 0.f)
        throw P3dError("optimizer: lr and momentum must be finite and momentum not negative");
    HIPCHECK(hipSetDevice(h->cfg.device));
    if (kind != h->opt_kind) {      // a fresh optimiser: zero slots, step 0
        HIPCHECK(hipStreamSynchronize(h->stream));
        HIPCHECK(hipStreamSynchronize(h->side_stream));
        HIPCHECK(hipStreamSynchronize(h->comm_stream));
        HIPCHECK(hipMemsetAsync(h->flat_m, 0, (size_t)h->n_train * 4, h->stream));
        HIPCHECK(hipMemsetAsync(h->flat_v, 0, (size_t)h->n_train * 4, h->stream));
        HIPCHECK(hipStreamSynchronize(h->stream));
        h->step = 0;
    }
    h->opt_kind = kind;
    h->lr = lr;
    h->momentum = momentum;
    h->use_nesterov = use_nesterov ? 1 : 0;
    API_END
}

// an optimiser slot of a trainable variable: its range of flat_m (slot 0) or flat_v (slot 1)
static float* slot_ptr(p3d_handle* h, const char* var, int slot, int64_t count) {
    Param* p = find_param(h, var, count);
    if (!p->trainable) throw P3dError(std::string(var) + " is not trainable: it has no optimiser slots");
    const int nslots = h->opt_kind == P3D_OPT_ADAM ? 2 : h->opt_kind == P3D_OPT_MOMENTUM ? 1 : 0;
    if (slot < 0 || slot >= nslots)
        throw P3dError("slot " + std::to_string(slot) + ": the current optimiser has " + std::to_string(nslots) + " slot(s)");
    return (slot == 0 ? h->flat_m : h->flat_v) + p->off;
}

int p3d_get_slot(p3d_handle* h, const char* var, int slot, float* host, int64_t count) {
    API_BEGIN
    if (!host) throw P3dError("null argument");
    float* d = slot_ptr(h, var, slot, count);
    HIPCHECK(hipSetDevice(h->cfg.device));
    HIPCHECK(copy_now(host, d, (size_t)count * 4, hipMemcpyDeviceToHost, h->stream));
    API_END
}

int p3d_set_slot(p3d_handle* h, const char* var, int slot, const float* host, int64_t count) {
    API_BEGIN
    if (!host) throw P3dError("null argument");
    float* d = slot_ptr(h, var, slot, count);
    HIPCHECK(hipSetDevice(h->cfg.device));
    HIPCHECK(hipStreamSynchronize(h->stream));      // as p3d_set_param: nothing else orders this copy after a running step
    HIPCHECK(hipStreamSynchronize(h->side_stream));
    HIPCHECK(hipStreamSynchronize(h->comm_stream));
    HIPCHECK(copy_now(d, host, (size_t)count * 4, hipMemcpyHostToDevice, h->stream));
    API_END
}

int p3d_get_optimizer_step(p3d_handle* h, int64_t* t) {
    API_BEGIN
    if (!h || !t) throw P3dError("null argument");
    *t = h->step;
    API_END
}

int p3d_set_optimizer_step(p3d_handle* h, int64_t t) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    if (t < 0) throw P3dError("optimizer step " + std::to_string(t) + " is negative");
    h->step = t;
    API_END
}

int p3d_activation_info(p3d_handle* h, const char* name, int64_t shape[5]) {
    API_BEGIN
    if (!h || !name) throw P3dError("null argument");
    auto it = h->named.find(name);
    if (it == h->named.end()) throw P3dError(std::string("no activation named ") + name);
    Act* a = it->second;
    shape[0] = a->N; shape[1] = a->D; shape[2] = a->H; shape[3] = a->W; shape[4] = a->C;
    API_END
}

int p3d_get_activation(p3d_handle* h, const char* name, float* host, int64_t count) {
    API_BEGIN
    if (!h || !name || !host) throw P3dError("null argument");
    auto it = h->named.find(name);
    if (it == h->named.end()) throw P3dError(std::string("no activation named ") + name);
    Act* a = it->second;
    if (count != a->rows() * a->C) throw P3dError("activation size mismatch");
    HIPCHECK(hipSetDevice(h->cfg.device));
    if (a->materialize && h->last_forward_fused) a->materialize(h->stream);
    h->download_act(a, host);
    API_END
}

int p3d_block_info(p3d_handle* h, int block_id, int64_t in_shape[5], int64_t out_shape[5]) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    auto it = h->blocks.find(block_id);
    if (it == h->blocks.end()) throw P3dError("no bottleneck with id " + std::to_string(block_id));
    const Act* a = it->second.in; const Act* b = it->second.out;
    if (in_shape) { in_shape[0] = a->N; in_shape[1] = a->D; in_shape[2] = a->H; in_shape[3] = a->W; in_shape[4] = a->C; }
    if (out_shape) { out_shape[0] = b->N; out_shape[1] = b->D; out_shape[2] = b->H; out_shape[3] = b->W; out_shape[4] = b->C; }
    API_END
}

int p3d_block_forward(p3d_handle* h, int block_id, const float* in, int64_t in_count, float* out, int64_t out_count) {
    API_BEGIN
    if (!h || !in || !out) throw P3dError("null argument");
    auto it = h->blocks.find(block_id);
    if (it == h->blocks.end()) throw P3dError("no bottleneck with id " + std::to_string(block_id));
    Act* a = it->second.in; Act* b = it->second.out;
    if (in_count != a->rows() * a->C || out_count != b->rows() * b->C) throw P3dError("block tensor size mismatch");
    HIPCHECK(hipSetDevice(h->cfg.device));
    HIPCHECK(hipMemcpy2DAsync(a->p, (size_t)a->ld * 4, in, (size_t)a->C * 4, (size_t)a->C * 4, (size_t)a->rows(), hipMemcpyHostToDevice, h->stream));
    Ctx c; c.training = true; c.s = h->stream; c.fuse = h->fuse_bn;
    h->last_forward_fused = c.fuse;
    h->sib_pending.clear();
    if (h->stats_count) HIPCHECK(hipMemsetAsync(h->stats_arena, 0, (size_t)h->stats_count * sizeof(double), c.s));
    for (size_t i = it->second.op0; i < it->second.op1; ++i) h->ops[i].fwd(c);      // (no zero arena: ops zero what they slice)
    h->download_act(b, out);
    API_END
}

int p3d_block_backward(p3d_handle* h, int block_id, const float* in, int64_t in_count, const float* dout, int64_t out_count, float* din) {
    API_BEGIN
    if (!h || !in || !dout || !din) throw P3dError("null argument");
    auto it = h->blocks.find(block_id);
    if (it == h->blocks.end()) throw P3dError("no bottleneck with id " + std::to_string(block_id));
    Act* a = it->second.in; Act* b = it->second.out;
    if (in_count != a->rows() * a->C || out_count != b->rows() * b->C) throw P3dError("block tensor size mismatch");
    if (!a->g || !b->g) throw P3dError("this bottleneck's input or output carries no gradient");
    HIPCHECK(hipSetDevice(h->cfg.device));
    HIPCHECK(hipMemcpy2DAsync(a->p, (size_t)a->ld * 4, in, (size_t)a->C * 4, (size_t)a->C * 4, (size_t)a->rows(), hipMemcpyHostToDevice, h->stream));
    Ctx c; c.training = true; c.s = h->stream; c.fuse = false;
    h->sib_pending.clear();
    h->last_forward_fused = false;
    if (h->stats_count) HIPCHECK(hipMemsetAsync(h->stats_arena, 0, (size_t)h->stats_count * sizeof(double), c.s));
    for (size_t i = it->second.op0; i < it->second.op1; ++i) h->ops[i].fwd(c);
    // the backward walk of run_backward over this block's ops only, on one stream; the block's output gradient is given
    h->zeroed_early = false;
    h->zero_backward_arenas(c.s, true);
    c.z0 = h->zb; c.z1 = h->zb + h->zb_bytes;
    HIPCHECK(hipMemcpy2DAsync(b->g, (size_t)b->ld * 4, dout, (size_t)b->C * 4, (size_t)b->C * 4, (size_t)b->rows(), hipMemcpyHostToDevice, c.s));
    h->wq.clear(); h->wq_flushes = 0; h->parked_flops = 0;
    for (size_t i = it->second.op1; i-- > it->second.op0;) {
        c.bwd_op = h->ops[i].name.c_str();
        h->ops[i].bwd(c);
    }
    h->flush_wgrads(c);
    HIPCHECK(hipMemcpy2DAsync(din, (size_t)a->C * 4, a->g, (size_t)a->ld * 4, (size_t)a->C * 4, (size_t)a->rows(), hipMemcpyDeviceToHost, c.s));
    HIPCHECK(hipStreamSynchronize(c.s));
    API_END
}

int p3d_profile_step(p3d_handle* h, float dropout_rate, uint64_t seed, p3d_op_time* out, int cap) {
    if (!h) { g_err = "null handle"; return -1; }
    try {
        h->refuse_swapped("p3d_profile_step");
        HIPCHECK(hipSetDevice(h->cfg.device));
        PerturbPause unperturbed;
        Prof prof;
        Ctx c; c.training = true; c.drop = dropout_rate; c.seed = seed; c.update_moving = true; c.s = h->stream; c.prof = &prof;
        prof.phase = 0; h->run_forward(c);
        prof.cur_op = "loss"; h->run_loss(c);
        // no collective here: bench.py profiles on rank 0 only, after the timed region -- an all-reduce that the
        // other ranks do not enter would never return
        if (h->acc_accumulating()) {      // a micro-step of p3d_set_grad_accum that only accumulates
            prof.phase = 1; h->run_backward(c, false);
            prof.phase = 2; prof.cur_op = "grad_accum"; h->grad_accum_take(c);
        } else {
            c.acc_finish = h->acc_k > 1;
            prof.phase = 1; h->run_backward(c, false);
            prof.phase = 2; prof.cur_op = "adam"; h->run_adam(c);
            h->acc_pending = 0;
        }
        HIPCHECK(hipStreamSynchronize(c.s));
        int w = 0;
        for (auto& r : prof.recs) {
            float ms = 0;
            HIPCHECK(hipEventElapsedTime(&ms, r.e0, r.e1));
            if (w < cap && out) {
                p3d_op_time& o = out[w];
                memset(&o, 0, sizeof(o));
                snprintf(o.name, sizeof(o.name), "%s", r.op.c_str());
                snprintf(o.kernel, sizeof(o.kernel), "%s", r.kernel.c_str());
                o.ms = ms; o.flops = r.flops; o.bytes = r.bytes; o.phase = r.phase;
            }
            ++w;
            hipEventDestroy(r.e0);
            hipEventDestroy(r.e1);
        }
        return w;
    } catch (const std::exception& e) {
        g_err = e.what();
        return -1;
    }
}

int p3d_debug_bucket_audit(p3d_handle* h, float dropout_rate, uint64_t seed, int64_t bucket_floats, int64_t* lo, int64_t* hi,
                           int32_t* after_op, int cap, int64_t* n_train, int64_t* stale) {
    if (!h) { g_err = "null handle"; return -1; }
    int count = 0;
    try {
        HIPCHECK(hipSetDevice(h->cfg.device));
        if (bucket_floats < 1) throw P3dError("bucket size must be positive");
        struct Snap { int64_t lo, hi; int op; std::vector<float> g; };
        std::vector<Snap> snaps;
        const int64_t saved = h->bucket_floats;
        h->bucket_floats = bucket_floats;
        h->bucket_hook = [&](int64_t l, int64_t u, int op) {
            // everything the bucket's gradients depend on must already be QUEUED: wait for it, then look
            HIPCHECK(hipStreamSynchronize(h->stream));
            HIPCHECK(hipStreamSynchronize(h->side_stream));
            Snap s; s.lo = l; s.hi = u; s.op = op; s.g.resize((size_t)(u - l));
            HIPCHECK(copy_now(s.g.data(), h->flat_g + l, (size_t)(u - l) * 4, hipMemcpyDeviceToHost, h->stream));
            snaps.push_back(std::move(s));
        };
        try {
            Ctx c; c.training = true; c.drop = dropout_rate; c.seed = seed; c.update_moving = false; c.s = h->stream;
            h->run_forward(c);
            h->run_loss(c);
            h->run_backward(c, true);
            HIPCHECK(hipStreamSynchronize(h->stream));
            HIPCHECK(hipStreamSynchronize(h->side_stream));
        } catch (...) {
            h->bucket_hook = nullptr; h->bucket_floats = saved;
            throw;
        }
        h->bucket_hook = nullptr; h->bucket_floats = saved;
        std::vector<float> fin((size_t)h->n_train);
        HIPCHECK(copy_now(fin.data(), h->flat_g, (size_t)h->n_train * 4, hipMemcpyDeviceToHost, h->stream));
        int64_t bad = 0;
        for (auto& s : snaps) {
            if (memcmp(s.g.data(), fin.data() + s.lo, s.g.size() * 4) != 0)
                for (size_t i = 0; i < s.g.size(); ++i)
                    if (memcmp(&s.g[i], &fin[(size_t)s.lo + i], 4) != 0) ++bad;
            if (count < cap) {
                if (lo) lo[count] = s.lo;
                if (hi) hi[count] = s.hi;
                if (after_op) after_op[count] = s.op;
            }
            ++count;
        }
        if (n_train) *n_train = h->n_train;
        if (stale) *stale = bad;
    } catch (const std::exception& e) {
        g_err = e.what();
        return -1;
    }
    return count;
}

int p3d_comm_unique_id(void* id_out) {
    API_BEGIN
    static_assert(sizeof(ncclUniqueId) <= P3D_COMM_ID_BYTES, "id size");
    ncclUniqueId id;
    NCCLCHECK(ncclGetUniqueId(&id));
    memset(id_out, 0, P3D_COMM_ID_BYTES);
    memcpy(id_out, &id, sizeof(id));
    API_END
}

int p3d_comm_init(p3d_handle* h, const void* idbytes) {
    API_BEGIN
    if (!h || !idbytes) throw P3dError("null argument");
    if (h->cfg.world_size < 1) throw P3dError("bad world_size");      // world_size 1 is allowed (single-rank communicator, for tests)
    HIPCHECK(hipSetDevice(h->cfg.device));
    ncclUniqueId id;
    memcpy(&id, idbytes, sizeof(id));
    NCCLCHECK(ncclCommInitRank(&h->comm, h->cfg.world_size, id, h->cfg.rank));
    if (const long mb = bucket_mb_env(); mb >= 1) h->bucket_floats = (int64_t)mb * (1 << 18);
    API_END
}

int p3d_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { hipGetLastError(); return -1; }
    return n;
}

int p3d_comm_info(p3d_handle* h, int* n_ranks, int* rank, int* device) {
    API_BEGIN
    if (!h) throw P3dError("null handle");
    int n = 0, r = -1, d = h->cfg.device;
    if (h->comm) {
        NCCLCHECK(ncclCommCount(h->comm, &n));
        NCCLCHECK(ncclCommUserRank(h->comm, &r));
        NCCLCHECK(ncclCommCuDevice(h->comm, &d));
    }
    if (n_ranks) *n_ranks = n;
    if (rank) *rank = r;
    if (device) *device = d;
    API_END
}

// ---- single-operator entry points ------------------------------------------------------------------
namespace {
// The single-operator entry points launch on the null stream (Ctx::s == nullptr), and so do their buffers: n elements (at least
// one), uploaded from `host` when given.
extern "C++" {
template <typename T>
struct DevArr : DevMem<T> {
    explicit DevArr(size_t n, const T* host = nullptr) : DevMem<T>(n > 0 ? n : 1, "no device memory for an op-level buffer") {
        if (host) HIPCHECK(copy_now(this->p, host, n * sizeof(T), hipMemcpyHostToDevice, nullptr));
    }
    void get(T* host, size_t n) { HIPCHECK(hipDeviceSynchronize()); HIPCHECK(copy_now(host, this->p, n * sizeof(T), hipMemcpyDeviceToHost, nullptr)); }
};
}
// floats, zero where nothing is uploaded
struct DevBuf : DevArr<float> {
    explicit DevBuf(int64_t n, const float* host = nullptr) : DevArr<float>((size_t)(n > 0 ? n : 0), host) {
        if (!host) HIPCHECK(fill_now(p, 0, this->n * 4, nullptr));
    }
};
int64_t prod5(const int64_t s[5]) { return s[0] * s[1] * s[2] * s[3] * s[4]; }
bool is_stem_shape(const int64_t xs[5], const int64_t ws[5]) { return xs[4] % 4 != 0 && ws[0] == 1; }
// One conv on dense tensors of the given shapes, described the way conv() / deconv() describe theirs: geometry, channel counts, rows
// of the conv's output and its forward launches.  transpose: xs is the input of tf.layers.conv3d_transpose and ws its kernel
// [kd,kh,kw,Cout,Cin].  The stem ([1,kh,kw,3,C]) runs on its packed form `sg` and reads the packed copies x4 / w4 (stem_pack).
struct ConvProblem {
    ConvGeo g; int N = 0, Cin = 0, Cout = 0; int64_t rows = 0, rows_in = 0; bool transpose = false, stem = false; StemGeo sg{};
    int64_t ny() const { return rows * Cout; }
    // ldx / ldy: floats per row of x and y where they are channel slices of wider rows (0: dense)
    std::vector<IgemmArgs> forward(const float* x, const float* w, float* y, const float* bias, const float* x4 = nullptr,
                                   const float* w4 = nullptr, int ldx = 0, int ldy = 0, int accum = 0) const {
        if (!ldx) ldx = Cin;
        if (!ldy) ldy = Cout;
        if (transpose) return igemm_conv_input_side(g, N, x, ldx, Cin, y, ldy, Cout, w, bias, 0, true);
        if (stem) return {stem_forward_args(sg, x4, w4, y, Cout, bias)};
        return {igemm_conv_forward(g, N, x, ldx, Cin, y, ldy, Cout, w, bias, accum)};
    }
    // the gradient of the conv's input from the gradient of its output, as conv()'s backward sends it: residue classes without
    // a tap are written (zeros) only when nothing is accumulated
    std::vector<IgemmArgs> input_gradient(const float* dy, const float* w, float* dx, int lddy = 0, int lddx = 0, int accum = 0) const {
        return igemm_conv_input_side(g, N, dy, lddy ? lddy : Cout, Cout, dx, lddx ? lddx : Cin, Cin, w, nullptr, accum, /*include_empty=*/!accum);
    }
    // the filter gradient as conv() / deconv() queue it (transpose: x is the transposed conv's input, dy the gradient of its output)
    WgradArgs filter_gradient(const float* x, int ldx, const float* dy, int lddy, float* dw, float* dbias) const {
        if (transpose) return wgrad_conv(g, N, dy, lddy, Cout, x, ldx, Cin, dw, nullptr);
        return wgrad_conv(g, N, x, ldx, Cin, dy, lddy, Cout, dw, dbias);
    }
};
ConvProblem conv_problem(const int64_t xs[5], const int64_t ws[5], const int s[3], int transpose) {
    ConvProblem r;
    const int k[3] = {(int)ws[0], (int)ws[1], (int)ws[2]};
    r.N = (int)xs[0]; r.Cin = (int)xs[4]; r.transpose = transpose != 0;
    r.rows_in = xs[0] * xs[1] * xs[2] * xs[3];
    if (transpose) {
        r.Cout = (int)ws[3];
        if (ws[4] != r.Cin) throw P3dError("kernel Cin mismatch");
        r.g = make_geo((int)xs[1] * s[0], (int)xs[2] * s[1], (int)xs[3] * s[2], k, s);      // the conv whose input is the output
        r.rows = xs[0] * r.g.I[0] * r.g.I[1] * r.g.I[2];
        return r;
    }
    r.Cout = (int)ws[4];
    r.g = make_geo((int)xs[1], (int)xs[2], (int)xs[3], k, s);
    r.rows = xs[0] * r.g.O[0] * r.g.O[1] * r.g.O[2];
    r.stem = is_stem_shape(xs, ws);
    if (r.stem) r.sg = stem_geo(r.g, r.N, r.Cout);
    return r;
}
}  // namespace

// ---- decisions of the last forward (test hook, include/p3d_hip.h) ---------------------------------------------------------
static const Op* decision_op(p3d_handle* h, int index) {
    if (!h) throw P3dError("null handle");
    int k = 0;
    for (const Op& op : h->ops)
        if (!op.dec_kind.empty() && k++ == index) return &op;
    throw P3dError("no decision site " + std::to_string(index));
}
int p3d_debug_decision_count(p3d_handle* h) {
    if (!h) return -1;
    int k = 0;
    for (const Op& op : h->ops) k += !op.dec_kind.empty();
    return k;
}
int p3d_debug_decision_info(p3d_handle* h, int index, const char** kind, const char** name1, const char** name2, int64_t shape[5]) {
    API_BEGIN
    const Op* op = decision_op(h, index);
    if (kind) *kind = op->dec_kind.c_str();
    if (name1) *name1 = op->dec_name1.c_str();
    if (name2) *name2 = op->dec_name2.c_str();
    const Act* a = op->dec_act;
    if (shape) { shape[0] = a->N; shape[1] = a->D; shape[2] = a->H; shape[3] = a->W; shape[4] = a->C; }
    API_END
}
int p3d_debug_decision_get(p3d_handle* h, int index, float* out1, float* out2, int64_t count) {
    API_BEGIN
    const Op* op = decision_op(h, index);
    const Act* a = op->dec_act;
    if (!out1 || count != a->rows() * a->C) throw P3dError("decision buffer size mismatch");
    HIPCHECK(hipSetDevice(h->cfg.device));
    HIPCHECK(hipStreamSynchronize(h->stream));
    if (op->dec_kind == "pool") {
        h->download_act(const_cast<Act*>(a), out1);
    } else {
        if (h->last_forward_fused) throw P3dError("decisions are read from the stored tensors: run the forward with BatchNorm fusion off");
        std::vector<float> ones((size_t)count, 1.0f);
        DevBuf d1(count, ones.data()), o1(count), o2(count), scratch(std::max<int64_t>(op->dec_scratch, 4 * (int64_t)a->C + 64));
        // DevBuf zero-fills on the NULL stream; the handle's stream is non-blocking and would not wait for those fills
        // (they would land on top of what the kernels below write)
        HIPCHECK(hipDeviceSynchronize());
        op->gates(h->stream, d1.p, o1.p, o2.p, scratch.p);
        o1.get(out1, count);
        if (out2) o2.get(out2, count);
    }
    API_END
}

int p3d_op_conv3d(int device, const float* x, const int64_t xs[5], const float* w, const int64_t ws[5], const int s[3],
                  const float* bias, float* y) {
    API_BEGIN
    HIPCHECK(hipSetDevice(device));
    const ConvProblem p = conv_problem(xs, ws, s, 0);
    DevBuf dx(prod5(xs), x), dw(prod5(ws), w), dy(p.ny()), db(p.Cout, bias), x4(p.sg.x4_floats), w4(p.sg.w4_floats);
    ensure_zero_page();
    Ctx c;
    if (p.stem) {          // [1,kh,kw,3,Cout] on its packed form, like the network's stem
        if (p.Cin != 3) throw P3dError("conv3d: channel counts that are not multiples of 4 are supported for the 3-channel stem only");
        stem_pack(c, p.sg, dx.p, x4.p, dw.p, w4.p);
    }
    auto v = p.forward(dx.p, dw.p, dy.p, bias ? db.p : nullptr, x4.p, w4.p);
    run_igemm_group(c, v, false, nullptr);
    if (p.stem) HIPCHECK(hipDeviceSynchronize());
    dy.get(y, p.ny());
    API_END
}

int p3d_op_conv3d_backprop_input(int device, const float* dyh, const float* w, const int64_t ws[5], const int s[3],
                                 const int64_t xs[5], float* dxh) {
    API_BEGIN
    HIPCHECK(hipSetDevice(device));
    const ConvProblem p = conv_problem(xs, ws, s, 0);
    DevBuf dy(p.ny(), dyh), dw(prod5(ws), w), dx(prod5(xs));
    auto v = p.input_gradient(dy.p, dw.p, dx.p);
    ensure_zero_page();
    { Ctx c; run_igemm_group(c, v, false, nullptr); }
    dx.get(dxh, prod5(xs));
    API_END
}

int p3d_op_conv3d_backprop_filter(int device, const float* x, const int64_t xs[5], const float* dyh, const int64_t ws[5],
                                  const int s[3], float* dwh, float* dbh) {
    API_BEGIN
    HIPCHECK(hipSetDevice(device));
    const ConvProblem p = conv_problem(xs, ws, s, 0);
    const int Cin = p.Cin, Cout = p.Cout;
    DevBuf dx(prod5(xs), x), dy(p.ny(), dyh), dw(prod5(ws)), db(Cout);
    ensure_zero_page();
    Ctx c;
    if (p.stem) {          // [1,kh,kw,3,Cout] on its packed form, like the network's stem (no atomics anywhere)
        if (Cin != 3) throw P3dError("conv3d_backprop_filter: channel counts that are not multiples of 4 are supported for the 3-channel stem only");
        DevBuf x4(p.sg.x4_floats), dw4(p.sg.w4_floats), spart(p.sg.part_floats);
        stem_pack(c, p.sg, dx.p, x4.p);
        if (p.sg.part_floats) {      // the network's stem: one pass (stem_wgrad.hip)
            stem_filter_gradient(c, p.sg, x4.p, dy.p, Cout, dw4.p, dw.p, nullptr, false, spart.p);
            if (dbh) HIPCHECK(p3d_colsum(dy.p, Cout, p.rows, Cout, db.p, c.s));
        } else
        stem_filter_gradient(c, p.sg, x4.p, dy.p, Cout, dw4.p, dw.p, dbh ? db.p : nullptr, false);
        HIPCHECK(hipDeviceSynchronize());
    } else {
        launch_wgrad(c, p.filter_gradient(dx.p, Cin, dy.p, Cout, dw.p, dbh ? db.p : nullptr));
    }
    dw.get(dwh, prod5(ws));
    if (dbh) db.get(dbh, Cout);
    API_END
}

// Test hook (ADVICE round 4): the stem's filter gradient THROUGH its BatchNorm + ReLU -- stem_wgrad.hip's FUSED form, which evaluates
// bn_bwd_apply_kernel<0> on the kernel's B operand -- beside the two-launch form (bn_bwd_apply, then the plain one-pass filter
// gradient), on the same inputs.  x [N,D,H,W,3]; y, dz [N,D,Ho,Wo,64] (the conv output and the gradient of relu(bn(y)));
// tab = scale, shift, mean, invstd, gamma [5][64]; coef [64][2] = (sum g / M, sum g*xhat / M); batch 1 / 0 = batch / moving statistics.
int p3d_debug_stem_wgrad_through_bn(int device, const float* x, const int64_t xs[5], const float* y, const float* dz, const float* tab,
                                    const float* coef, int batch, float* dw_fused, float* dw_two_launches) {
    API_BEGIN
    HIPCHECK(hipSetDevice(device));
    if (!x || !y || !dz || !tab || !coef || !dw_fused || !dw_two_launches) throw P3dError("null argument");
    const int64_t ws[5] = {1, 7, 7, 3, 64};
    const int s[3] = {1, 2, 2};
    const ConvProblem cp = conv_problem(xs, ws, s, 0);
    const StemGeo& sg = cp.sg;
    if (xs[4] != 3 || !sg.part_floats) throw P3dError("not a stem shape the one-pass kernel takes");
    const int Cout = cp.Cout;
    const int64_t rows = cp.rows, ny = cp.ny(), nw = prod5(ws);
    DevBuf dx(prod5(xs), x), dyb(ny, y), dzb(ny, dz), tb(5 * Cout, tab), cf(2 * Cout, coef), dyo(ny), dw1(nw), dw2(nw);
    ensure_zero_page();
    DevBuf x4(sg.x4_floats), dw4(sg.w4_floats), spart(sg.part_floats);
    Ctx c;
    stem_pack(c, sg, dx.p, x4.p);
    BnPass p;
    p.mode = 0; p.M = rows; p.C = Cout; p.dz = dzb.p; p.lddz = Cout; p.y1 = dyb.p; p.ld1 = Cout; p.dy1 = dyo.p; p.lddy1 = Cout;
    p.bn[0] = bn_layout(tb.p + 4 * Cout, nullptr, nullptr, nullptr, tb.p, nullptr, 0, Cout);
    p.coef[0] = cf.p; p.batch[0] = batch ? 1 : 0;
    const BnBwdArgs a = bn_bwd_args(p);
    stem_filter_gradient(c, sg, x4.p, nullptr, Cout, dw4.p, dw1.p, nullptr, false, spart.p, &a);       // fused
    HIPCHECK(p3d_bn_bwd_apply(a, c.s));                                                                                           // two launches
    stem_filter_gradient(c, sg, x4.p, dyo.p, Cout, dw4.p, dw2.p, nullptr, false, spart.p, nullptr);
    HIPCHECK(hipDeviceSynchronize());
    dw1.get(dw_fused, nw);
    dw2.get(dw_two_launches, nw);
    API_END
}

// ---- BatchNorm statistics behind a conv (test hooks, include/p3d_hip.h) ----------------------------------------------------
namespace {
// A conv that feeds a BatchNorm: what conv() / deconv() refuse is refused here.
ConvProblem conv_bn_problem(const int64_t xs[5], const int64_t ws[5], const int s[3], int transpose, bool bias) {
    const ConvProblem p = conv_problem(xs, ws, s, transpose);
    if (!transpose && ws[3] != p.Cin) throw P3dError("filter Cin mismatch");
    if (p.stem && (p.Cin != 3 || bias)) throw P3dError("the stem path is for [1,kh,kw,3,C] kernels without bias");
    return p;
}
int group_parts(const std::vector<IgemmArgs>& v) {
    int n = 0;
    for (const IgemmArgs& a : v) n += p3d_igemm2_mtiles(a, p3d_igemm2_plan(a, 1));
    return n;
}
}  // namespace

int p3d_debug_stat_parts(const int64_t xs[5], const int64_t ws[5], const int s[3], int transpose, int* written, int* cap) {
    API_BEGIN
    if (!xs || !ws || !s || !written || !cap) throw P3dError("null argument");
    const ConvProblem p = conv_bn_problem(xs, ws, s, transpose, false);
    const bool small = p3d_bn_small_ok((long)p.rows, p.Cout);      // (the network's stats_target: no epilogue partials)
    *written = small ? 0 : group_parts(p.forward(nullptr, nullptr, nullptr, nullptr));
    *cap = small ? 0 : bn_part_cap(p.rows, p.Cout);
    API_END
}

int p3d_debug_igemm_groupable(const int64_t xs[5], const int64_t ws[5], const int s[3]) {
    try {
        if (!xs || !ws || !s) throw P3dError("null argument");
        // two sibling convs of one input, as conv() sends them (ST_B): distinct weights and outputs, shared everything else
        static float dummy[4];
        const ConvProblem p = conv_bn_problem(xs, ws, s, 0, false);
        if (p.stem) throw P3dError("the stem has no sibling");
        std::vector<IgemmArgs> v{p.forward(dummy, dummy, dummy, nullptr)[0], p.forward(dummy, dummy + 1, dummy + 2, nullptr)[0]};
        return p3d_igemm2_groupable(v.data(), 2, p3d_igemm2_plan(v[0], 1)) ? 1 : 0;
    } catch (const std::exception& e) {
        g_err = e.what();
        return -1;
    }
}

int p3d_debug_conv_bn_stats(int device, const float* x, const int64_t xs[5], const float* w, const float* w2, const int64_t ws[5],
                            const int s[3], const float* bias, int transpose, float* moving, float* y, float* y2, float* stats,
                            int* nparts, const char** kernel) {
    API_BEGIN
    HIPCHECK(hipSetDevice(device));
    if (!x || !w || !xs || !ws || !s || !moving || !y || !stats || !nparts) throw P3dError("null argument");
    if (w2 && (transpose || !y2)) throw P3dError("a sibling pair is two forward convs with two outputs");
    const int64_t nx = prod5(xs), nw = prod5(ws);
    const ConvProblem p = conv_bn_problem(xs, ws, s, transpose, bias != nullptr);
    const int C = p.Cout, npair = w2 ? 2 : 1;
    const int64_t rows = p.rows, ny = p.ny();
    DevBuf dx(nx, x), dw(nw, w), dw2(w2 ? nw : 1, w2), dy(ny), dy2(w2 ? ny : 1), db(C, bias);
    std::vector<float> ones((size_t)C, 1.0f);
    DevBuf gamma(C, ones.data()), beta(C), mv(2 * (int64_t)C * npair, moving), tab(4 * (int64_t)C * npair);
    ensure_zero_page();
    Ctx c;
    DevBuf x4(p.sg.x4_floats), w4(p.sg.w4_floats);
    if (p.stem) stem_pack(c, p.sg, dx.p, x4.p, dw.p, w4.p);
    std::vector<IgemmArgs> v = p.forward(dx.p, dw.p, dy.p, bias ? db.p : nullptr, x4.p, w4.p);
    // the network's rule (stats_target): a tensor the one-launch small-tensor BatchNorm consumes gets no epilogue partials --
    // the statistics below then come from p3d_bn_stats
    const bool small = p3d_bn_small_ok((long)rows, C);
    const int cap = bn_part_cap(rows, C);
    DevBuf part((int64_t)cap * C * 2 * npair);
    int np[2] = {0, 0};
    const P3dIgemmPlan pl = p3d_igemm2_plan(v[0], 1);
    if (kernel) *kernel = v.size() == 1 && p3d_igemm2_tail_split(v[0], pl) ? "igemm2_group_kernel(tail)" : pl.name;
    if (!w2) {
        StatSink sink; sink.part = part.p; sink.cap = cap; sink.nparts = &np[0];
        run_igemm_group(c, v, false, small ? nullptr : &sink);
    } else {
        // conv()'s sibling pair
        v.push_back(p.forward(dx.p, dw2.p, dy2.p, bias ? db.p : nullptr)[0]);
        for (int q = 0; q < 2; ++q) {
            StatSink sink; sink.part = part.p + (int64_t)q * cap * C * 2; sink.cap = cap; sink.nparts = &np[q];
            sibling_prepare(v[q], small ? nullptr : &sink);
        }
        if (launch_siblings(c, v) && kernel) *kernel = "igemm2_group_kernel(siblings)";
    }
    for (int q = 0; q < npair; ++q) {
        float* pq = part.p + (int64_t)q * cap * C * 2;
        if (small) {
            if (p3d_bn_stats_parts((long)rows, C) > cap) throw P3dError("statistics partials overflow their arena slot");
            HIPCHECK(p3d_bn_stats(q ? dy2.p : dy.p, C, (long)rows, C, pq, c.s));
            np[q] = p3d_bn_stats_parts((long)rows, C);
        }
        float* m = mv.p + (int64_t)q * 2 * C;
        HIPCHECK(p3d_bn_finalize(bn_layout(gamma.p, beta.p, m, m + C, tab.p + (int64_t)q * 4 * C, pq, np[q], C), (long)rows, 1, 1, 1e-3f, c.s));
        nparts[q] = small ? 0 : np[q];
    }
    dy.get(y, ny);
    if (w2) dy2.get(y2, ny);
    mv.get(moving, 2 * (int64_t)C * npair);
    tab.get(stats, 4 * (int64_t)C * npair);
    API_END
}

// One normalise / ReLU / add pass of bn_apply (net_ops.inc) on raw inputs, forward and then backward, through the path rule and
// launch sequences the network itself calls (bn_path, bn_pass_forward / bn_pass_backward, net.hip).  The operands are C-channel
// slices of wider rows, as the network's are of its conv outputs and concat buffers, and the pass drops out as a dropout site's
// does (set_dropout).  The statistics of the non-small paths come from p3d_bn_stats, standing in for the producer's epilogue.
int p3d_debug_bn_pass(int device, int mode, int64_t M, int C, const float* y1, int ld1, int off1, const float* y2, int ld2, int off2,
                      const float* params, int batch1, int batch2, int update_moving, const float* dz, int acc2, float drop_rate,
                      uint64_t seed, int seed_dev, int path, float* z, int ldz, int offz, float* dy1, float* dy2, float* grads,
                      float* moving, int* info) {
    API_BEGIN
    HIPCHECK(hipSetDevice(device));
    if (mode < 0 || mode > 4) throw P3dError("bn_pass: mode must be 0..4");
    const bool two = (mode == 2 || mode == 3), has2 = mode != 0;
    const int nbn = two ? 2 : 1;
    if (!y1 || !params || !dz || !z || !dy1 || !grads || !moving || !info || (has2 && (!y2 || !dy2))) throw P3dError("null argument");
    if (M < 1 || C < 4 || C > 1024 || (C & 3) || path < 0 || path > 3) throw P3dError("bn_pass: bad shape or path");
    auto slice_ok = [&](int ld, int off) { return !(ld & 3) && !(off & 3) && off >= 0 && ld >= off + C; };
    if (!slice_ok(ld1, off1) || !slice_ok(ldz, offz) || (has2 && !slice_ok(ld2, off2)))
        throw P3dError("bn_pass: row strides and channel offsets are multiples of 4 with offset + C <= stride");
    if (!(drop_rate >= 0.f && drop_rate < 1.f)) throw P3dError("bn_pass: dropout rate must be in [0, 1)");
    const bool dropout = drop_rate > 0.f;
    const float drop_scale = dropout ? 1.f / (1.f - drop_rate) : 0.f;      // (set_dropout's)
    const bool b1 = batch1 != 0, b2 = two && batch2 != 0;
    const int sparts = p3d_bn_stats_parts((long)M, C), bparts = p3d_bn_bwd_parts((long)M, C);
    // the network's rule, or the forced path -- which must be one the kernels take (a pass that drops out takes only finalize + apply)
    const int taken = path ? path : bn_path(M, C, dropout, b1 ? sparts : 0, b2 ? sparts : 0, drop_scale);
    if (taken == BN_SMALL && (dropout || !p3d_bn_small_ok((long)M, C)))
        throw P3dError("bn_pass: the small-tensor path does not take this shape, or a pass that drops out");
    if (taken == BN_FOLD && !p3d_bn_fold_apply_ok((long)M, C, b1 ? sparts : 0, b2 ? sparts : 0, drop_scale))
        throw P3dError("bn_pass: the fold-apply path does not take this shape, or a pass that drops out");
    const int64_t n1 = M * ld1, n2 = has2 ? M * ld2 : 1, nz = M * ldz;
    DevBuf dy1b(n1, y1), dy2b(n2, has2 ? y2 : nullptr), dzb(nz, dz), zb(nz, z), g1(n1, dy1), g2(n2, has2 ? dy2 : nullptr);
    DevBuf prm(2 * (int64_t)C * nbn, params), mv(2 * (int64_t)C * nbn, moving), tab(4 * (int64_t)C * nbn), grd(2 * (int64_t)C * nbn);
    DevBuf spart((int64_t)sparts * 2 * C * nbn), bpart((int64_t)bparts * 2 * C * nbn), coef(2 * (int64_t)C * nbn);
    DevBuf dseed(2);
    HIPCHECK(copy_now(dseed.p, &seed, sizeof(seed), hipMemcpyHostToDevice, nullptr));
    Ctx c;         // (bn_apply at a dropout site: the step's seed as an argument or in device memory)
    c.training = true; c.drop = drop_rate;
    if (seed_dev) c.seed_dev = reinterpret_cast<const unsigned long long*>(dseed.p); else c.seed = seed;
    BnPass p;
    p.mode = mode; p.M = M; p.C = C; p.nparts = bparts;
    p.y1 = dy1b.p + off1; p.ld1 = ld1; p.z = zb.p + offz; p.ldz = ldz; p.dz = dzb.p + offz; p.lddz = ldz; p.dy1 = g1.p + off1; p.lddy1 = ld1;
    if (has2) { p.y2 = dy2b.p + off2; p.ld2 = ld2; p.dy2 = g2.p + off2; p.lddy2 = ld2; p.acc2 = acc2 ? 1 : 0; }
    for (int q = 0; q < nbn; ++q) {
        const int64_t o = (int64_t)q * 2 * C;
        p.bn[q] = bn_layout(prm.p + o, prm.p + o + C, mv.p + o, mv.p + o + C, tab.p + 2 * o, spart.p + o * sparts, sparts, C);
        p.dgamma[q] = grd.p + o; p.dbeta[q] = grd.p + o + C; p.part[q] = bpart.p + o * bparts; p.coef[q] = coef.p + o;
        p.batch[q] = q ? b2 : b1;
        if (taken != BN_SMALL && p.batch[q]) HIPCHECK(p3d_bn_stats(q ? p.y2 : p.y1, q ? ld2 : ld1, (long)M, C, spart.p + o * sparts, c.s));
    }
    set_dropout(p, c, dropout);
    bn_pass_forward(c, p, (BnPath)taken, update_moving != 0);
    bn_pass_backward(c, p, taken == BN_SMALL);
    info[0] = taken; info[1] = taken == BN_SMALL ? 0 : sparts; info[2] = taken == BN_SMALL ? 0 : bparts;
    zb.get(z, nz);
    g1.get(dy1, n1);
    if (has2) g2.get(dy2, n2);
    grd.get(grads, 2 * (int64_t)C * nbn);
    mv.get(moving, 2 * (int64_t)C * nbn);
    API_END
}

// One GroupNorm pass of gn_apply (net_gn.inc) on raw inputs, forward and then backward, through the launch sequences the network
// itself calls (gn_pass_forward / gn_pass_backward, net.hip).
int p3d_debug_gn_pass(int device, int mode, int N, int R, int C, int G, float eps, const float* y1, int ld1, const float* y2, int ld2,
                      int ldz, const float* params, const float* cs, const float* ss, const float* dz, int acc2, float drop_rate,
                      uint64_t seed, int path, float* z, float* dy1, float* dy2, float* grads, float* tables, int* info) {
    API_BEGIN
    HIPCHECK(hipSetDevice(device));
    if (mode < 0 || mode > 6) throw P3dError("gn_pass: mode must be 0..6");
    const bool two = (mode == 2 || mode == 3), has2 = mode != 0 && mode != 5, bwd = mode != 2;
    const bool d2 = mode == 1 || mode == 3 || mode == 4 || mode == 6;      // a second input gradient
    const int ngn = two ? 2 : 1;
    if (!y1 || !params || !z || !dy1 || !grads || !tables || !info || (has2 && !y2) || (bwd && !dz) || (bwd && d2 && !dy2) ||
        (mode == 6 && (!cs || !ss)))
        throw P3dError("null argument");
    if (N < 1 || R < 1 || C < 4 || C > 1024 || (C & 3) || G < 1 || C % G || path < 0 || path > 2)
        throw P3dError("gn_pass: bad shape or path");
    if (ld1 < C || (ld1 & 3) || ldz < C || (ldz & 3) || (has2 && (ld2 < C || (ld2 & 3))))
        throw P3dError("gn_pass: row strides must be multiples of 4, at least C");
    if (!(drop_rate >= 0.f && drop_rate < 1.f)) throw P3dError("gn_pass: dropout rate must be in [0, 1)");
    const int64_t M = (int64_t)N * R, nc = (int64_t)N * C;
    const bool dropout = drop_rate > 0.f;
    // the network's rule, or the forced path -- which must be one the kernels take
    const bool small_ok = mode != 2 && !dropout && p3d_gn_small_ok(R, C, G);
    const int taken = path ? path : (gn_small_rule(mode, R, C, G, two ? G : 0, dropout) ? 1 : 2);
    if (taken == 1 && !small_ok) throw P3dError("gn_pass: the small-tensor path does not take this shape");
    DevBuf y1b(M * ld1, y1), y2b(has2 ? M * ld2 : 1, has2 ? y2 : nullptr), zb(M * ldz, z), dzb(bwd ? M * ldz : 1, bwd ? dz : nullptr);
    DevBuf g1b(M * ld1, dy1), g2b(bwd && d2 ? M * ld2 : 1, bwd && d2 ? dy2 : nullptr);
    DevBuf prm(2 * (int64_t)C * ngn, params), grd(2 * (int64_t)C * ngn, grads), tab(7 * nc * ngn);
    DevBuf csb(mode == 6 ? nc : 1, mode == 6 ? cs : nullptr), ssb(mode == 6 ? M : 1, mode == 6 ? ss : nullptr);
    DevBuf fsums(4 * nc * ngn), bsums(4 * nc * ngn);           // [gn][N][C][2] doubles each: forward, backward (as the arenas)
    Ctx c;
    c.training = true; c.drop = drop_rate; c.seed = seed;
    auto args = [&](bool backward) {
        GnOperand o[2];
        o[0].y = y1b.p; o[0].ld = ld1; o[0].dy = g1b.p; o[0].lddy = ld1;
        if (has2) { o[1].y = y2b.p; o[1].ld = ld2; }
        if (d2) { o[1].dy = g2b.p; o[1].lddy = ld2; }
        for (int q = 0; q < ngn; ++q) {
            float* const w = prm.p + (int64_t)q * 2 * C; float* const dw = grd.p + (int64_t)q * 2 * C;
            double* const sums = reinterpret_cast<double*>(backward ? bsums.p : fsums.p) + (int64_t)q * 2 * nc;
            o[q].g = gn_layout(w, w + C, sums, tab.p + (int64_t)q * 7 * nc, N, C, G);
            o[q].dgamma = dw; o[q].dbeta = dw + C;
        }
        return gn_apply_args(mode, M, R, C, eps, o[0], o[1], (d2 && acc2) ? 1 : 0, mode == 6 ? csb.p : nullptr, mode == 6 ? ssb.p : nullptr,
                             zb.p, ldz, dzb.p, c, dropout);
    };
    gn_pass_forward(c, args(false), taken == 1);
    if (bwd) gn_pass_backward(c, args(true), taken == 1);
    info[0] = taken;
    zb.get(z, M * ldz);
    if (bwd) {
        g1b.get(dy1, M * ld1);
        if (d2) g2b.get(dy2, M * ld2);
        grd.get(grads, 2 * (int64_t)C * ngn);
    }
    std::vector<float> t((size_t)(7 * nc * ngn));
    tab.get(t.data(), 7 * nc * ngn);
    for (int q = 0; q < ngn; ++q) std::copy(t.begin() + q * 7 * nc, t.begin() + q * 7 * nc + 4 * nc, tables + q * 4 * nc);
    API_END
}

// CBAM forward and backward on raw inputs, through the argument builder and the launches cbam() (net_gn.inc) itself uses, with the
// network's chunk rule unless chunks > 0.
int p3d_debug_cbam(int device, int N, int D, int H, int W, int C, const float* x, int ld, const float* k0, const float* b0,
                   const float* k1, const float* b1, const float* k7, int chunks, const float* dout, int accx, float* cs, float* sp,
                   float* ss, float* dx, float* pgrads, int* info) {
    API_BEGIN
    HIPCHECK(hipSetDevice(device));
    if (!x || !k0 || !b0 || !k1 || !b1 || !k7 || !dout || !cs || !sp || !ss || !dx || !pgrads || !info) throw P3dError("null argument");
    if (N < 1 || D < 1 || H < 1 || W < 1 || C < 8 || C > 1024 || (C & 3) || chunks < 0 || chunks > 65535)
        throw P3dError("cbam: bad shape or chunk count");
    if (ld < C || (ld & 3)) throw P3dError("cbam: the row stride must be a multiple of 4, at least C");
    const int R = D * H * W, Ch = C / 8;
    const int64_t M = (int64_t)N * R, nc = (int64_t)N * C;
    const int64_t ng = (int64_t)C * Ch * 2 + Ch + C + 686;      // dk0, db0, dk1, db1, dk7
    const int nchunks = chunks ? chunks : cbam_chunks(R);
    const CbamLayout L = cbam_layout(N, M, C, nchunks);
    DevBuf xb(M * ld, x), k0b((int64_t)C * Ch, k0), b0b(Ch, b0), k1b((int64_t)Ch * C, k1), b1b(C, b1), k7b(686, k7);
    DevBuf doutb(M * C, dout), dxb(M * ld, dx), grd(ng, pgrads), scratch(L.total);
    const float* const w[5] = {k0b.p, b0b.p, k1b.p, b1b.p, k7b.p};
    float* const dk0 = grd.p; float* const db0 = dk0 + (int64_t)C * Ch; float* const dk1 = db0 + Ch; float* const db1 = dk1 + (int64_t)Ch * C;
    float* const dw[5] = {dk0, db0, dk1, db1, db1 + C};
    const CbamArgs a = cbam_args(N, D, H, W, C, xb.p, ld, w, nchunks, scratch.p, doutb.p, dxb.p, accx ? 1 : 0, dw);
    Ctx c;
    cbam_pass_forward(c, a);
    cbam_pass_backward(c, a);
    std::vector<float> h((size_t)L.total);
    scratch.get(h.data(), L.total);
    std::copy(h.begin() + L.cs, h.begin() + L.cs + nc, cs);
    std::copy(h.begin() + L.sp, h.begin() + L.sp + 2 * M, sp);
    std::copy(h.begin() + L.ss, h.begin() + L.ss + M, ss);
    dxb.get(dx, M * ld);
    grd.get(pgrads, ng);
    info[0] = a.chunks;
    API_END
}

// The output head on raw inputs: forward, filter gradient and input gradient through the argument builder and the launches head()
// (net_graphs.inc) itself uses, on their rule or on a forced kernel.
int p3d_debug_head(int device, int transpose, int N, int D, int H, int W, int C, const float* x, const float* k, const float* bias,
                   int sigmoid, const float* dlogits, int fwd_path, int filter_path, float* logits, float* pred, float* dx, float* dk,
                   float* dbias, int* info) {
    API_BEGIN
    HIPCHECK(hipSetDevice(device));
    if (!x || !k || !bias || !dlogits || !logits || !pred || !dx || !dk || !dbias || !info) throw P3dError("null argument");
    if (N < 1 || D < 1 || H < 1 || W < 1 || C < 1) throw P3dError("head: bad shape");
    if (!transpose && (fwd_path || filter_path)) throw P3dError("head: the stride-1 head has one kernel per pass");
    const int up = transpose ? 2 : 1;
    const int64_t M = (int64_t)N * D * H * W, Mo = M * up * up * up;
    DevBuf xb(M * C, x), kb(27 * (int64_t)C, k), bb(1, bias), lb(Mo), pb(Mo), dlb(Mo, dlogits), dxb(M * C), dkb(27 * (int64_t)C, dk),
        dbb(1, dbias);
    const HeadArgs a = head_args(xb.p, N, D, H, W, C, kb.p, bb.p, lb.p, pb.p, sigmoid ? 1 : 0, dlb.p, dxb.p, dkb.p, dbb.p);
    HeadLaunch f{0, 0}, w{0, 0};
    Ctx c;
    head_forward(c, a, transpose != 0, fwd_path, &f);
    head_filter_gradient(c, a, transpose != 0, filter_path, &w);
    head_input_gradient(c, a, transpose != 0);
    lb.get(logits, Mo);
    pb.get(pred, Mo);
    dxb.get(dx, M * C);
    dkb.get(dk, 27 * (int64_t)C);
    dbb.get(dbias, 1);
    info[0] = f.kernel; info[1] = (int)f.blocks; info[2] = w.kernel; info[3] = (int)w.blocks;
    API_END
}

// ---- the loss and optimiser hooks: the launches run_loss and adam_range (net_sched.inc) issue, on raw inputs -------------------
namespace {
// n floats placed `offset` elements into a zeroed device buffer, uploaded from `host` when given
struct StagedBuf : DevBuf {
    int64_t n; int offset;
    StagedBuf(int64_t n_, int offset_, const float* host = nullptr) : DevBuf(n_ + offset_), n(n_), offset(offset_) {
        if (host) HIPCHECK(copy_now(at(), host, (size_t)n * 4, hipMemcpyHostToDevice, nullptr));
    }
    float* at() const { return p + offset; }
    void back(float* host) const { if (host) HIPCHECK(copy_now(host, at(), (size_t)n * 4, hipMemcpyDeviceToHost, nullptr)); }
};
// a double the launch adds into or writes: up from *host, and back
struct StagedDouble : DevBuf {
    explicit StagedDouble(const double* host) : DevBuf(2) { HIPCHECK(copy_now(p, host, sizeof(double), hipMemcpyHostToDevice, nullptr)); }
    double* at() const { return reinterpret_cast<double*>(p); }
    void back(double* host) const { HIPCHECK(copy_now(host, p, sizeof(double), hipMemcpyDeviceToHost, nullptr)); }
};

// p3d_loss under kind 0, 1 or 2 (logits may be null under kind 0, which never reads them)
void debug_loss(int device, int kind, const float* logits, const float* pred, const float* target, int64_t n, int through_sigmoid,
                int offset, double* loss, float* dlogits, int* info, const char* what) {
    HIPCHECK(hipSetDevice(device));
    if ((kind != P3D_LOSS_SMOOTH_L1 && !logits) || !pred || !target || !loss || !dlogits || !info) throw P3dError("null argument");
    if (n < 1 || offset < 0 || offset > 3) throw P3dError(std::string(what) + ": bad length or offset");
    StagedBuf zb(n, offset, logits), pb(n, offset, pred), tb(n, offset, target), db(n, offset);
    StagedDouble lb(loss);
    const LossArgs a{kind, zb.at(), pb.at(), tb.at(), (long)n, through_sigmoid ? 1 : 0, lb.at(), db.at()};
    unsigned done[2] = {0, 0};
    HIPCHECK(p3d_loss(a, nullptr, done));
    HIPCHECK(hipDeviceSynchronize());
    db.back(dlogits);
    lb.back(loss);
    info[0] = (int)done[0]; info[1] = (int)done[1];
}

// the tile table of a decay hook: tiles must cover [0, n) in order
std::vector<P3dRegTile> host_tiles(const int64_t* tile_off, const int64_t* tile_len, const float* tile_c, int ntile, int64_t n,
                                   const char* what) {
    std::vector<P3dRegTile> tiles((size_t)ntile);
    int64_t at = 0;
    bool ok = true;
    for (int k = 0; k < ntile && ok; ++k) {
        ok = tile_off[k] == at && tile_len[k] >= 1 && tile_len[k] <= (1 << 30);
        tiles[k] = {(long long)tile_off[k], (int)tile_len[k], tile_c[k]};
        at += tile_len[k];
    }
    if (!ok || at != n) throw P3dError(std::string(what) + ": tiles must cover [0, n) in order");
    return tiles;
}

// p3d_opt_step: `a` brings the update and its hyper-parameters; p, g, m, v are the host's arrays (null: a zeroed buffer, not
// copied back; g_out null: the gradient is not copied back), n elements each, `offset` elements into the device buffers.  step: the
// step size, as an argument or (lr_on_device) through device memory as a captured step reads it.  tiles: the decay part, with
// the whole table folded into *term.
void debug_opt_step(OptArgs a, float* p, const float* g, float* g_out, float* m, float* v, int64_t n, int offset,
                    float step, int lr_on_device, const std::vector<P3dRegTile>& tiles = {}, double* term = nullptr,
                    const float* gscale = nullptr) {
    const int64_t ntile = (int64_t)tiles.size();
    StagedBuf pb(n, offset, p), gb(n, offset, g), mb(n, offset, m), vb(n, offset, v);
    DevBuf lrb(1), tb(4 * ntile), part(2 * ntile), scal(4);      // scal (zeroed): [0..1] the term, [2] the fold's counter
    a.p = pb.at(); a.g = gb.at(); a.m = mb.at(); a.v = vb.at(); a.n = (long)n;
    if (lr_on_device) HIPCHECK(p3d_set_step_scalars(nullptr, lrb.p, nullptr, 0, step, 0.f, nullptr));
    DevBuf sc(1, gscale);      // clipping's scale, read from device memory as the step reads it
    if (gscale) a.gscale = sc.p;
    // from device memory the argument must not matter: NaN would show in every element if the kernel read it
    a.lr = lr_on_device ? NAN : step;
    a.lr_dev = lr_on_device ? lrb.p : nullptr;
    if (ntile) {
        HIPCHECK(copy_now(tb.p, tiles.data(), tiles.size() * sizeof(P3dRegTile), hipMemcpyHostToDevice, nullptr));
        a.tiles = reinterpret_cast<P3dRegTile*>(tb.p); a.ntile = (int)ntile; a.tile_base = 0;
        a.part = reinterpret_cast<double*>(part.p); a.fold_part = a.part; a.nfold = (int)ntile;
        a.counter = reinterpret_cast<unsigned*>(scal.p + 2); a.term = reinterpret_cast<double*>(scal.p);
    }
    HIPCHECK(p3d_opt_step(a, nullptr));
    HIPCHECK(hipDeviceSynchronize());
    pb.back(p); gb.back(g_out); mb.back(m); vb.back(v);
    if (term) HIPCHECK(copy_now(term, scal.p, sizeof(double), hipMemcpyDeviceToHost, nullptr));
}
OptArgs adam_update(float b1, float b2, float eps, int update = 1) {
    OptArgs a;
    a.update = update ? UPD_ADAM : UPD_NONE; a.b1 = b1; a.b2 = b2; a.eps = eps;
    return a;
}
OptArgs momentum_update(int kind, float momentum, int use_nesterov, int update = 1) {
    OptArgs a;
    a.update = update ? kind : UPD_NONE; a.momentum = momentum; a.nesterov = use_nesterov;      // the gradient-only launch is the same under every kind
    return a;
}
}  // namespace

int p3d_debug_smooth_l1(int device, const float* pred, const float* target, int64_t n, int through_sigmoid, int offset, double* loss,
                        float* dlogits, int* info) {
    API_BEGIN
    debug_loss(device, P3D_LOSS_SMOOTH_L1, nullptr, pred, target, n, through_sigmoid, offset, loss, dlogits, info, "smooth_l1");
    API_END
}

int p3d_debug_loss(int device, int kind, const float* logits, const float* pred, const float* target, int64_t n, int through_sigmoid,
                   int offset, double* loss, float* dlogits, int* info) {
    API_BEGIN
    if (kind == P3D_LOSS_KLD_CC) throw P3dError("loss: kind 3 (per-map KL + CC) needs the map geometry: p3d_debug_map_loss");
    if (kind == P3D_LOSS_SALIENCY) throw P3dError("loss: kind 4 (per-map KL + CC + NSS + SIM) needs the map geometry: p3d_debug_saliency_loss");
    if (kind != P3D_LOSS_SMOOTH_L1 && kind != P3D_LOSS_BCE && kind != P3D_LOSS_L1) throw P3dError("loss: kind is 0, 1 or 2");
    debug_loss(device, kind, logits, pred, target, n, through_sigmoid, offset, loss, dlogits, info, kind ? "loss" : "smooth_l1");
    API_END
}

// The per-map loss (run_map_loss in net_sched.inc) on raw inputs, placed as p3d_debug_loss places them, with scratch sized and
// zeroed as the handle plans it.
int p3d_debug_map_loss(int device, const float* logits, const float* pred, const float* target, int64_t maps, int64_t map_elems,
                       int through_sigmoid, int offset, float kld_weight, float cc_weight, double* loss, float* dlogits,
                       double* per_map, int* info) {
    API_BEGIN
    HIPCHECK(hipSetDevice(device));
    if (!logits || !target || !loss || !dlogits || !per_map || !info || (through_sigmoid && !pred)) throw P3dError("null argument");
    if (maps < 1 || map_elems < 1 || offset < 0 || offset > 3) throw P3dError("map loss: bad geometry or offset");
    if (maps * map_elems > ((int64_t)1 << 31)) throw P3dError("map loss: more than 2^31 elements");
    const int64_t n = maps * map_elems;
    size_t md = 0, mc = 0;
    p3d_map_loss_scratch(maps, map_elems, &md, &mc);
    StagedBuf zb(n, offset, logits), pb(n, offset, through_sigmoid ? pred : nullptr), tb(n, offset, target), db(n, offset);
    StagedDouble lb(loss);
    DevBuf sb(2 * (int64_t)md), cb((int64_t)mc);
    double* scratch = reinterpret_cast<double*>(sb.p);
    const MapLossArgs a = p3d_map_loss_args(zb.at(), pb.at(), tb.at(), maps, map_elems, through_sigmoid ? 1 : 0, kld_weight, cc_weight,
                                            lb.at(), db.at(), scratch, reinterpret_cast<unsigned*>(cb.p));
    for (int stage = 0; stage < 3; ++stage) HIPCHECK(p3d_map_loss_launch(stage, a, nullptr));
    HIPCHECK(hipDeviceSynchronize());
    std::vector<double> ms((size_t)maps * P3D_MAP_STATS);
    HIPCHECK(copy_now(ms.data(), scratch, ms.size() * sizeof(double), hipMemcpyDeviceToHost, nullptr));
    std::vector<unsigned> cnt(mc);
    HIPCHECK(copy_now(cnt.data(), cb.p, mc * sizeof(unsigned), hipMemcpyDeviceToHost, nullptr));
    for (unsigned v : cnt)
        if (v) throw P3dError("map loss: an arrival counter was left nonzero");
    for (int64_t m = 0; m < maps; ++m) {
        per_map[2 * m] = ms[(size_t)m * P3D_MAP_STATS + 2];
        per_map[2 * m + 1] = ms[(size_t)m * P3D_MAP_STATS + 3];
    }
    db.back(dlogits);
    lb.back(loss);
    info[0] = 3; info[1] = a.blocks; info[2] = a.vec4 ? 1 : 2;
    API_END
}

// The same for P3D_LOSS_SALIENCY (run_saliency_loss): the fixation bytes sit `offset` bytes into their buffer.
int p3d_debug_saliency_loss(int device, const float* logits, const float* pred, const float* target, const unsigned char* fix,
                            int64_t maps, int64_t map_elems, int through_sigmoid, int offset, float kld_weight, float cc_weight,
                            float nss_weight, float sim_weight, double* loss, float* dlogits, double* per_map, int* info) {
    API_BEGIN
    HIPCHECK(hipSetDevice(device));
    if (!logits || !target || !loss || !dlogits || !per_map || !info || (through_sigmoid && !pred) || (nss_weight > 0.f && !fix))
        throw P3dError("null argument");
    if (maps < 1 || map_elems < 1 || offset < 0 || offset > 3) throw P3dError("saliency loss: bad geometry or offset");
    if (maps * map_elems > ((int64_t)1 << 31)) throw P3dError("saliency loss: more than 2^31 elements");
    for (float w : {kld_weight, cc_weight, nss_weight, sim_weight})
        if (!std::isfinite(w) || w < 0.f) throw P3dError("saliency loss weights must be finite and not negative");
    const int64_t n = maps * map_elems;
    size_t md = 0, mc = 0;
    p3d_saliency_loss_scratch(maps, map_elems, &md, &mc);
    StagedBuf zb(n, offset, logits), pb(n, offset, through_sigmoid ? pred : nullptr), tb(n, offset, target), db(n, offset);
    DevBuf fb((n + offset + 3) / 4 + 1);      // the bytes, in a zeroed buffer of whole words
    unsigned char* fdev = reinterpret_cast<unsigned char*>(fb.p) + offset;
    if (fix) HIPCHECK(copy_now(fdev, fix, (size_t)n, hipMemcpyHostToDevice, nullptr));
    StagedDouble lb(loss);
    DevBuf sb(2 * (int64_t)md), cb((int64_t)mc);
    double* scratch = reinterpret_cast<double*>(sb.p);
    const SaliencyLossArgs a = p3d_saliency_loss_args(zb.at(), pb.at(), tb.at(), fdev, maps, map_elems, through_sigmoid ? 1 : 0, kld_weight,
                                                      cc_weight, nss_weight, sim_weight, lb.at(), db.at(), scratch,
                                                      reinterpret_cast<unsigned*>(cb.p));
    for (int stage = 0; stage < 3; ++stage) HIPCHECK(p3d_saliency_loss_launch(stage, a, nullptr));
    HIPCHECK(hipDeviceSynchronize());
    std::vector<double> st((size_t)maps * (P3D_MAP_STATS + P3D_SAL_STATS));
    HIPCHECK(copy_now(st.data(), scratch, st.size() * sizeof(double), hipMemcpyDeviceToHost, nullptr));
    std::vector<unsigned> cnt(mc);
    HIPCHECK(copy_now(cnt.data(), cb.p, mc * sizeof(unsigned), hipMemcpyDeviceToHost, nullptr));
    for (unsigned v : cnt)
        if (v) throw P3dError("saliency loss: an arrival counter was left nonzero");
    const double* xs = st.data() + (size_t)maps * P3D_MAP_STATS;
    for (int64_t m = 0; m < maps; ++m) {
        per_map[4 * m] = st[(size_t)m * P3D_MAP_STATS + 2];
        per_map[4 * m + 1] = st[(size_t)m * P3D_MAP_STATS + 3];
        per_map[4 * m + 2] = xs[(size_t)m * P3D_SAL_STATS + 6];
        per_map[4 * m + 3] = xs[(size_t)m * P3D_SAL_STATS + 7];
    }
    db.back(dlogits);
    lb.back(loss);
    info[0] = 3; info[1] = a.m.blocks; info[2] = a.m.vec4 ? 1 : 2;
    API_END
}

// Adam: the step size for step t comes from adam_step_size, and is returned in *lr_t.
int p3d_debug_adam(int device, float* p, const float* g, float* m, float* v, int64_t n, int offset, float lr, int64_t t, float b1,
                   float b2, float eps, int lr_on_device, float* lr_t) {
    API_BEGIN
    HIPCHECK(hipSetDevice(device));
    if (!p || !g || !m || !v || !lr_t) throw P3dError("null argument");
    if (n < 1 || t < 1 || offset < 0 || offset > 3) throw P3dError("adam: bad length, step or offset");
    const float step = adam_step_size(lr, b1, b2, t);
    debug_opt_step(adam_update(b1, b2, eps), p, g, nullptr, m, v, n, offset, step, lr_on_device);
    *lr_t = step;
    API_END
}

// Momentum / SGD, placed as p3d_debug_adam places its buffers.
int p3d_debug_optimizer(int device, int kind, float* p, float* g, float* m, int64_t n, int offset, float lr, float momentum,
                        int use_nesterov, int lr_on_device) {
    API_BEGIN
    HIPCHECK(hipSetDevice(device));
    if (!p || !g || !m) throw P3dError("null argument");
    if (kind != P3D_OPT_MOMENTUM && kind != P3D_OPT_SGD) throw P3dError("optimizer: kind 1 (momentum) or 2 (sgd); Adam has p3d_debug_adam");
    if (n < 1 || offset < 0 || offset > 3) throw P3dError("optimizer: bad length or offset");
    debug_opt_step(momentum_update(kind, momentum, use_nesterov), p, g, g, m, nullptr, n, offset, lr, lr_on_device);
    API_END
}

// ema_kernel from the step's launch description.  The range sits `offset` elements past a 16-byte boundary with one guard element
// on each side of it in both buffers; a guard that the launch changed is an error.
int p3d_debug_ema(int device, float* s, const float* p, int64_t n, int offset, float om, int om_on_device) {
    API_BEGIN
    HIPCHECK(hipSetDevice(device));
    if (!s || !p) throw P3dError("null argument");
    if (n < 1 || offset < 0 || offset > 3) throw P3dError("ema: bad length or offset");
    const int64_t at = 4 + offset;
    const uint32_t guard = 0x7fc5a5a5u;      // a NaN no arithmetic here produces
    std::vector<uint32_t> gs((size_t)(n + 12), guard);
    DevBuf sb(n + 12, reinterpret_cast<const float*>(gs.data())), pb(n + 12, reinterpret_cast<const float*>(gs.data())), omb(1);
    HIPCHECK(copy_now(sb.p + at, s, (size_t)n * 4, hipMemcpyHostToDevice, nullptr));
    HIPCHECK(copy_now(pb.p + at, p, (size_t)n * 4, hipMemcpyHostToDevice, nullptr));
    if (om_on_device) HIPCHECK(p3d_set_step_scalars(nullptr, nullptr, omb.p, 0, 0.f, om, nullptr));
    EmaArgs a;
    a.s = sb.p + at; a.p = pb.p + at; a.n = (long)n;
    a.om = om_on_device ? NAN : om;      // from device memory the argument must not matter
    a.om_dev = om_on_device ? omb.p : nullptr;
    const LaunchDesc d = p3d_ema_desc(a);
    if (std::string(d.kernel) != "ema_kernel") throw P3dError("ema: launch description names another kernel");
    HIPCHECK(p3d_ema_step(a, nullptr));
    HIPCHECK(hipDeviceSynchronize());
    std::vector<uint32_t> back((size_t)(n + 12)), pback((size_t)(n + 12));
    HIPCHECK(copy_now(back.data(), sb.p, back.size() * 4, hipMemcpyDeviceToHost, nullptr));
    HIPCHECK(copy_now(pback.data(), pb.p, pback.size() * 4, hipMemcpyDeviceToHost, nullptr));
    for (int64_t i = 0; i < n + 12; ++i)
        if ((i < at || i >= at + n) && (back[(size_t)i] != guard || pback[(size_t)i] != guard))
            throw P3dError("ema: the launch wrote outside its range (element " + std::to_string(i - at) + ")");
    if (memcmp(pback.data() + at, p, (size_t)n * 4) != 0) throw P3dError("ema: the launch changed the parameters");
    memcpy(s, back.data() + at, (size_t)n * 4);
    API_END
}

// One grad_accum_kernel launch from the step's launch description, placed and guarded as p3d_debug_ema's.  The operand the mode
// writes comes back; the other one must keep its bits.
int p3d_debug_grad_accum(int device, int mode, float* acc, float* g, int64_t n, int offset) {
    API_BEGIN
    HIPCHECK(hipSetDevice(device));
    if (!acc || !g) throw P3dError("null argument");
    if (mode < GACC_STORE || mode > GACC_FINISH) throw P3dError("grad_accum: mode is 0 (store), 1 (add) or 2 (finish)");
    if (n < 1 || offset < 0 || offset > 3) throw P3dError("grad_accum: bad length or offset");
    const int64_t at = 4 + offset;
    const uint32_t guard = 0x7fc5a5a5u;      // a NaN no arithmetic here produces
    std::vector<uint32_t> gs((size_t)(n + 12), guard);
    DevBuf ab(n + 12, reinterpret_cast<const float*>(gs.data())), gb(n + 12, reinterpret_cast<const float*>(gs.data()));
    HIPCHECK(copy_now(ab.p + at, acc, (size_t)n * 4, hipMemcpyHostToDevice, nullptr));
    HIPCHECK(copy_now(gb.p + at, g, (size_t)n * 4, hipMemcpyHostToDevice, nullptr));
    GradAccumArgs a;
    a.acc = ab.p + at; a.g = gb.p + at; a.n = (long)n; a.mode = mode;
    const LaunchDesc d = p3d_grad_accum_desc(a);
    if (std::string(d.kernel) != "grad_accum_kernel<" + std::to_string(mode) + ">")
        throw P3dError("grad_accum: launch description names another kernel");
    HIPCHECK(p3d_grad_accum_step(a, nullptr));
    HIPCHECK(hipDeviceSynchronize());
    std::vector<uint32_t> aback((size_t)(n + 12)), gback((size_t)(n + 12));
    HIPCHECK(copy_now(aback.data(), ab.p, aback.size() * 4, hipMemcpyDeviceToHost, nullptr));
    HIPCHECK(copy_now(gback.data(), gb.p, gback.size() * 4, hipMemcpyDeviceToHost, nullptr));
    for (int64_t i = 0; i < n + 12; ++i)
        if ((i < at || i >= at + n) && (aback[(size_t)i] != guard || gback[(size_t)i] != guard))
            throw P3dError("grad_accum: the launch wrote outside its range (element " + std::to_string(i - at) + ")");
    if (mode == GACC_FINISH) {
        if (memcmp(aback.data() + at, acc, (size_t)n * 4) != 0) throw P3dError("grad_accum: FINISH changed the accumulator");
        memcpy(g, gback.data() + at, (size_t)n * 4);
    } else {
        if (memcmp(gback.data() + at, g, (size_t)n * 4) != 0) throw P3dError("grad_accum: the launch changed the gradient");
        memcpy(acc, aback.data() + at, (size_t)n * 4);
    }
    API_END
}

// The augmentation launches of p3d_set_augment from the step's launch builder, on explicit per-clip decisions.  Every buffer sits
// `offset` elements (bytes for the fixations) past a 16-byte boundary with guard elements on both sides; a guard or an input that
// the launches changed is an error.
int p3d_debug_augment(int device, const float* x, const float* y, const unsigned char* fix, int B, int T, int H, int W, const int32_t* geom,
                      const float* photo, int offset, float* x_out, float* y_out, unsigned char* fix_out) {
    API_BEGIN
    HIPCHECK(hipSetDevice(device));
    if (!x || !y || !geom || !photo || !x_out || !y_out || (fix && !fix_out)) throw P3dError("null argument");
    if (B < 1 || T < 1 || H < 1 || W < 1 || offset < 0 || offset > 3) throw P3dError("augment: bad shape or offset");
    const int64_t ne = (int64_t)B * T * H * W;
    if (ne * 3 > (int64_t)1 << 31) throw P3dError("augment: the hook takes up to 2^31 floats");
    std::vector<P3dAugClip> tab((size_t)B);
    for (int b = 0; b < B; ++b) {
        const int32_t* g = geom + 6 * b;
        tab[(size_t)b] = {g[0] != 0, g[1] != 0, g[2], g[3], g[4], g[5], photo[2 * b], photo[2 * b + 1]};
    }
    const int64_t at = 4 + offset, bat = 16 + offset;      // floats / bytes ahead of the ranges
    const uint32_t guard = 0x7fc5a5a5u;                    // a NaN no arithmetic here produces; its bytes guard the fixations
    auto guarded = [&](int64_t n, const float* host) {     // n floats at `at` of a buffer of guards
        std::vector<uint32_t> gs((size_t)(n + 12), guard);
        if (host) memcpy(gs.data() + at, host, (size_t)n * 4);
        return gs;
    };
    const int64_t bwords = (ne + 48 + 3) / 4;
    std::vector<uint32_t> fsrc((size_t)bwords, guard);
    if (fix) memcpy(reinterpret_cast<unsigned char*>(fsrc.data()) + bat, fix, (size_t)ne);
    const std::vector<uint32_t> xs = guarded(3 * ne, x), ys = guarded(ne, y), xo = guarded(3 * ne, nullptr), yo = guarded(ne, nullptr);
    const std::vector<uint32_t> fdst((size_t)bwords, guard);
    auto as_f = [](const std::vector<uint32_t>& v) { return reinterpret_cast<const float*>(v.data()); };
    DevBuf xsb(3 * ne + 12, as_f(xs)), ysb(ne + 12, as_f(ys)), xob(3 * ne + 12, as_f(xo)), yob(ne + 12, as_f(yo));
    DevBuf fsb(bwords, as_f(fsrc)), fob(bwords, as_f(fdst)), tb((int64_t)B * 8, reinterpret_cast<const float*>(tab.data()));
    static_assert(sizeof(P3dAugClip) == 32, "the table row is eight words");
    AugArgs a;
    a.x = xsb.p + at; a.y = ysb.p + at; a.x_out = xob.p + at; a.y_out = yob.p + at;
    if (fix) { a.fix = reinterpret_cast<unsigned char*>(fsb.p) + bat; a.fix_out = reinterpret_cast<unsigned char*>(fob.p) + bat; }
    a.tab = reinterpret_cast<const P3dAugClip*>(tb.p); a.tab_host = tab.data();
    a.B = B; a.T = T; a.H = H; a.W = W;
    static const char* const names[3] = {"augment_f32_kernel<3>", "augment_f32_kernel<1>", "augment_fix_kernel"};
    for (int st = 0; st < p3d_augment_stages(a); ++st) {
        if (std::string(p3d_augment_desc(st, a).kernel) != names[st]) throw P3dError("augment: launch description names another kernel");
        HIPCHECK(p3d_augment_launch(st, a, nullptr));
    }
    HIPCHECK(hipDeviceSynchronize());
    auto back = [&](const DevBuf& b, int64_t words) {
        std::vector<uint32_t> v((size_t)words);
        HIPCHECK(copy_now(v.data(), b.p, (size_t)words * 4, hipMemcpyDeviceToHost, nullptr));
        return v;
    };
    const std::vector<uint32_t> xs2 = back(xsb, 3 * ne + 12), ys2 = back(ysb, ne + 12), fs2 = back(fsb, bwords);
    if (xs2 != xs || ys2 != ys || fs2 != fsrc) throw P3dError("augment: the launches changed an input");
    const std::vector<uint32_t> xo2 = back(xob, 3 * ne + 12), yo2 = back(yob, ne + 12), fo2 = back(fob, bwords);
    auto guards_kept = [&](const std::vector<uint32_t>& v, int64_t n) {
        for (int64_t i = 0; i < (int64_t)v.size(); ++i)
            if ((i < at || i >= at + n) && v[(size_t)i] != guard) return false;
        return true;
    };
    if (!guards_kept(xo2, 3 * ne) || !guards_kept(yo2, ne)) throw P3dError("augment: a launch wrote outside its range");
    const unsigned char* fb = reinterpret_cast<const unsigned char*>(fo2.data());
    const unsigned char* gb = reinterpret_cast<const unsigned char*>(fdst.data());
    for (int64_t i = 0; i < bwords * 4; ++i)
        if ((i < bat || i >= bat + ne || !fix) && fb[i] != gb[i]) throw P3dError("augment: the fixation launch wrote outside its range");
    memcpy(x_out, xo2.data() + at, (size_t)ne * 12);
    memcpy(y_out, yo2.data() + at, (size_t)ne * 4);
    if (fix) memcpy(fix_out, fb + bat, (size_t)ne);
    API_END
}

// p3d_debug_adam_decay with Momentum / SGD as the update (update = 0 is the gradient-only launch).
int p3d_debug_optimizer_decay(int device, int kind, float* p, float* g, float* m, int64_t n, int offset, const int64_t* tile_off,
                              const int64_t* tile_len, const float* tile_c, int ntile, float lr, float momentum, int use_nesterov,
                              int lr_on_device, int update, double* term) {
    API_BEGIN
    HIPCHECK(hipSetDevice(device));
    if (!p || !g || !m || !tile_off || !tile_len || !tile_c || !term) throw P3dError("null argument");
    if (kind != P3D_OPT_MOMENTUM && kind != P3D_OPT_SGD)
        throw P3dError("optimizer_decay: kind 1 (momentum) or 2 (sgd); Adam has p3d_debug_adam_decay");
    if (n < 1 || offset < 0 || offset > 3 || ntile < 1) throw P3dError("optimizer_decay: bad length, offset or tile count");
    debug_opt_step(momentum_update(kind, momentum, use_nesterov, update), p, g, g, m, nullptr, n, offset, lr, lr_on_device,
                   host_tiles(tile_off, tile_len, tile_c, ntile, n, "optimizer_decay"), term);
    API_END
}

// The regularised launch on a tile table, placed as p3d_debug_adam places its buffers (update = 0 is the gradient-only launch).
int p3d_debug_adam_decay(int device, float* p, float* g, float* m, float* v, int64_t n, int offset, const int64_t* tile_off,
                         const int64_t* tile_len, const float* tile_c, int ntile, float lr, int64_t t, float b1, float b2, float eps,
                         int lr_on_device, int update, double* term, float* lr_t) {
    API_BEGIN
    HIPCHECK(hipSetDevice(device));
    if (!p || !g || !m || !v || !tile_off || !tile_len || !tile_c || !term || !lr_t) throw P3dError("null argument");
    if (n < 1 || t < 1 || offset < 0 || offset > 3 || ntile < 1) throw P3dError("adam_decay: bad length, step, offset or tile count");
    const std::vector<P3dRegTile> tiles = host_tiles(tile_off, tile_len, tile_c, ntile, n, "adam_decay");
    const float step = adam_step_size(lr, b1, b2, t);
    debug_opt_step(adam_update(b1, b2, eps, update), p, g, g, m, v, n, offset, step, lr_on_device, tiles, term);
    *lr_t = step;
    API_END
}

// Any optimiser launch with clipping's scale (p3d_debug_adam / _adam_decay / _optimizer / _optimizer_decay keep their arguments).
int p3d_debug_opt_scaled(int device, int kind, float* p, float* g, float* m, float* v, int64_t n, int offset, const int64_t* tile_off,
                         const int64_t* tile_len, const float* tile_c, int ntile, float lr, int64_t t, float b1, float b2, float eps,
                         float momentum, int use_nesterov, int lr_on_device, float gscale, double* term, float* lr_t) {
    API_BEGIN
    HIPCHECK(hipSetDevice(device));
    if (!p || !g || !m || !v || !lr_t || (ntile && (!tile_off || !tile_len || !tile_c || !term))) throw P3dError("null argument");
    if (kind != P3D_OPT_ADAM && kind != P3D_OPT_MOMENTUM && kind != P3D_OPT_SGD) throw P3dError("opt_scaled: kind 0, 1 or 2");
    if (n < 1 || t < 1 || offset < 0 || offset > 3 || ntile < 0) throw P3dError("opt_scaled: bad length, step, offset or tile count");
    std::vector<P3dRegTile> tiles;
    if (ntile) tiles = host_tiles(tile_off, tile_len, tile_c, ntile, n, "opt_scaled");
    const bool adam = kind == P3D_OPT_ADAM;
    const float step = adam ? adam_step_size(lr, b1, b2, t) : lr;
    debug_opt_step(adam ? adam_update(b1, b2, eps) : momentum_update(kind, momentum, use_nesterov), p, g, g, m, adam ? v : nullptr, n,
                   offset, step, lr_on_device, tiles, term, &gscale);
    *lr_t = step;
    API_END
}

// grad_sumsq_kernel on host arrays, through sumsq launches described as the step describes its own (SumsqArgs): chunks
// (chunk_off, chunk_len, chunk_c) ascending, gaps allowed (padding: never read); the ranges [range_lo, range_hi) are launched in
// the order given, the last one folding; together they must take every chunk once.
int p3d_debug_grad_norm(int device, const float* g, const float* p, int64_t n, int offset, const int64_t* chunk_off,
                        const int64_t* chunk_len, const float* chunk_c, int nchunk, const int64_t* range_lo, const int64_t* range_hi,
                        int nrange, float clip_norm, int max_blocks, double* sumsq, double* norm, float* scale) {
    API_BEGIN
    HIPCHECK(hipSetDevice(device));
    if (!g || !chunk_off || !chunk_len || !chunk_c || !range_lo || !range_hi || !sumsq || !norm || !scale) throw P3dError("null argument");
    if (n < 1 || offset < 0 || offset > 3 || nchunk < 1 || nrange < 1 || max_blocks < 0) throw P3dError("grad_norm: bad length, offset or counts");
    if (!(clip_norm > 0.f)) throw P3dError("grad_norm: clip_norm must be positive or +inf");
    std::vector<P3dRegTile> tiles((size_t)nchunk);
    int64_t at = 0;
    for (int k = 0; k < nchunk; ++k) {
        if (chunk_off[k] < at || chunk_len[k] < 1 || chunk_len[k] > (1 << 30) || chunk_off[k] + chunk_len[k] > n)
            throw P3dError("grad_norm: chunks must ascend without overlap inside [0, n)");
        if (chunk_c[k] != 0.f && !p) throw P3dError("grad_norm: a chunk has a coefficient but there are no parameters");
        tiles[(size_t)k] = {(long long)chunk_off[k], (int)chunk_len[k], chunk_c[k]};
        at = chunk_off[k] + chunk_len[k];
    }
    auto first_at = [&](int64_t off) {
        return (int)(std::lower_bound(tiles.begin(), tiles.end(), off, [](const P3dRegTile& t, int64_t o) { return t.off < o; }) - tiles.begin());
    };
    std::vector<int> taken((size_t)nchunk, 0);
    std::vector<std::pair<int, int>> cuts;
    for (int r = 0; r < nrange; ++r) {
        const int k0 = first_at(range_lo[r]), k1 = first_at(range_hi[r]);
        if (k1 <= k0 || tiles[(size_t)k1 - 1].off + tiles[(size_t)k1 - 1].len > range_hi[r]) throw P3dError("grad_norm: a range is empty or cuts a chunk");
        for (int k = k0; k < k1; ++k) ++taken[(size_t)k];
        cuts.push_back({k0, k1});
    }
    for (int k : taken) if (k != 1) throw P3dError("grad_norm: the ranges must take every chunk exactly once");
    StagedBuf gb(n, offset, g), pb(n, offset, p);
    DevBuf tb(4 * (int64_t)nchunk), part(2 * (int64_t)nchunk), res(8);      // res (zeroed): [0..5] the results, [6] the fold's counter
    HIPCHECK(copy_now(tb.p, tiles.data(), tiles.size() * sizeof(P3dRegTile), hipMemcpyHostToDevice, nullptr));
    for (int r = 0; r < nrange; ++r) {
        SumsqArgs a;
        a.g = gb.at(); a.p = p ? pb.at() : nullptr; a.tiles = reinterpret_cast<P3dRegTile*>(tb.p); a.tile_base = 0;
        a.k0 = cuts[(size_t)r].first; a.k1 = cuts[(size_t)r].second;
        a.part = reinterpret_cast<double*>(part.p); a.nfold = r == nrange - 1 ? nchunk : 0;
        a.counter = reinterpret_cast<unsigned*>(res.p + 6); a.res = reinterpret_cast<double*>(res.p);
        a.clip_norm = clip_norm; a.max_blocks = max_blocks;
        HIPCHECK(p3d_grad_sumsq(a, nullptr));
    }
    HIPCHECK(hipDeviceSynchronize());
    float back[8];
    HIPCHECK(copy_now(back, res.p, sizeof(back), hipMemcpyDeviceToHost, nullptr));
    if (reinterpret_cast<unsigned*>(back)[6]) throw P3dError("grad_norm: the arrival counter was left nonzero");
    memcpy(sumsq, back, 8); memcpy(norm, back + 2, 8); *scale = back[4];
    API_END
}

int p3d_op_conv3d_transpose(int device, const float* x, const int64_t xs[5], const float* kh, const int64_t ks[5],
                            const int s[3], const float* bias, float* y) {
    API_BEGIN
    HIPCHECK(hipSetDevice(device));
    const ConvProblem p = conv_problem(xs, ks, s, 1);
    DevBuf dx(prod5(xs), x), dk(prod5(ks), kh), dy(p.ny()), db(p.Cout, bias);
    auto v = p.forward(dx.p, dk.p, dy.p, bias ? db.p : nullptr);
    ensure_zero_page();
    { Ctx c; run_igemm_group(c, v, false, nullptr); }
    dy.get(y, p.ny());
    API_END
}

namespace {
// tf.nn.max_pool3d SAME and its gradient on host arrays whose rows of ldx / ldy floats hold the xs[4] channels at column offx / offy,
// through maxpool()'s launches (net_ops.inc).  y0 / dx0: what the output rows hold before (null: zeros; a slice keeps its other columns).
void max_pool3d_on_host_arrays(const float* x, int ldx, int offx, const int64_t xs[5], const int k[3], const int s[3], const float* y0,
                               float* y, int ldy, int offy) {
    const ConvGeo g = make_geo((int)xs[1], (int)xs[2], (int)xs[3], k, s);
    const int64_t rin = xs[0] * xs[1] * xs[2] * xs[3], rout = xs[0] * g.O[0] * g.O[1] * g.O[2];
    DevBuf dx(rin * ldx, x), dy(rout * ldy, y0);
    PoolArgs a = pool_args(g, (int)xs[0], (int)xs[4], ldx, ldy);
    a.x = dx.p + offx; a.y = dy.p + offy;
    pool_forward(Ctx(), a);
    dy.get(y, rout * ldy);
}
const char* max_pool3d_grad_on_host_arrays(const float* x, int ldx, int offx, const int64_t xs[5], const int k[3], const int s[3],
                                           const float* dyh, int ldy, int offy, int accumulate, const float* dx0, float* dxh) {
    const ConvGeo g = make_geo((int)xs[1], (int)xs[2], (int)xs[3], k, s);
    const int C = (int)xs[4];
    const int64_t rin = xs[0] * xs[1] * xs[2] * xs[3], rout = xs[0] * g.O[0] * g.O[1] * g.O[2];
    DevBuf dx(rin * ldx, x), dy(rout * ldy, dyh), dg(rin * ldx, dx0), yy(rout * ldy), tab(rout * (C / 4));
    PoolArgs a = pool_args(g, (int)xs[0], C, ldx, ldy);
    a.x = dx.p + offx; a.dy = dy.p + offy; a.dx = dg.p + offx; a.y = yy.p + offy;
    if (!p3d_maxpool_disjoint(a)) a.idx = reinterpret_cast<unsigned*>(tab.p);
    pool_forward(Ctx(), a);
    const char* const kernel = pool_backward(Ctx(), a, accumulate);
    dg.get(dxh, rin * ldx);
    return kernel;
}
// tf.nn.bias_add's gradient: dbias = db0 (null: zeros) + the column sums of `channels` columns at column `off` of rows of ld floats
void bias_add_grad_on_host_arrays(const float* dyh, int64_t rows, int channels, int ld, int off, const float* db0, float* dbias) {
    DevBuf dy(rows * ld, dyh), db(channels, db0);
    if (rows > 0) HIPCHECK(p3d_colsum(dy.p + off, ld, (long)rows, channels, db.p, nullptr));
    db.get(dbias, channels);
}
}  // namespace

int p3d_op_max_pool3d(int device, const float* x, const int64_t xs[5], const int k[3], const int s[3], float* y) {
    API_BEGIN
    HIPCHECK(hipSetDevice(device));
    max_pool3d_on_host_arrays(x, (int)xs[4], 0, xs, k, s, nullptr, y, (int)xs[4], 0);
    API_END
}

int p3d_op_max_pool3d_grad(int device, const float* x, const int64_t xs[5], const int k[3], const int s[3], const float* dyh,
                           float* dxh) {
    API_BEGIN
    HIPCHECK(hipSetDevice(device));
    if (xs[4] % 4) throw P3dError("max_pool3d_grad needs a channel count that is a multiple of 4");
    max_pool3d_grad_on_host_arrays(x, (int)xs[4], 0, xs, k, s, dyh, (int)xs[4], 0, 0, nullptr, dxh);
    API_END
}

int p3d_op_bias_add_grad(int device, const float* dyh, int64_t rows, int channels, float* dbias) {
    API_BEGIN
    if (!dyh || !dbias) throw P3dError("null argument");
    if (rows < 0 || channels < 1) throw P3dError("bias_add_grad needs rows >= 0 and channels >= 1");
    HIPCHECK(hipSetDevice(device));
    bias_add_grad_on_host_arrays(dyh, rows, channels, channels, 0, nullptr, dbias);
    API_END
}

// ---- launch forms of the train step (test hooks, include/p3d_hip.h) -------------------------------------------------------------
namespace {
// a channel slice of `C` floats at column `off` of rows of `ld` floats, as the kernels take it (float4 accesses)
void check_slice(const char* what, int ld, int off, int C) {
    if (C < 4 || (C & 3) || (ld & 3) || (off & 3) || off < 0 || ld < off + C)
        throw P3dError(std::string(what) + ": channels, row length and channel offset are multiples of 4 with offset + channels <= row length");
}
// the kernel names launch() was given while `f` ran, joined with ';'
void traced_kernels(const std::function<void()>& f, std::string& out) {
    SchedTrace tr;
    SchedTrace* const before = g_trace;
    g_trace = &tr;
    try { f(); } catch (...) { g_trace = before; throw; }
    g_trace = before;
    out.clear();
    for (const std::string& l : tr.lines) {
        if (l.compare(0, 2, "L ")) continue;
        const size_t sp = l.find(' ', 2);
        out += (out.empty() ? "" : ";") + l.substr(sp + 1);
    }
}
void put_string(const std::string& v, char* out, int cap) {
    if (!out || cap < 1) return;
    if ((int)v.size() >= cap) throw P3dError("kernel name buffer too small");
    memcpy(out, v.c_str(), v.size() + 1);
}
}  // namespace

int p3d_debug_perturb_selftest(int device, int mode, int slow, int delay_us, int with_wait, float* out) {
    API_BEGIN
    if (!out) throw P3dError("null argument");
    if (mode < 0 || mode > 2) throw P3dError("perturb: mode is 0 (off), 1 (serial) or 2 (slow)");
    if (mode == 2 && (slow < 0 || slow > 1)) throw P3dError("perturb self-test: slow is 0 (the producer's stream) or 1 (the consumer's)");
    if (mode == 2 && (delay_us < 1 || delay_us > 2000)) throw P3dError("perturb: delay_us must be in [1, 2000]");
    HIPCHECK(hipSetDevice(device));
    const int n = 4096;
    struct Streams {      // two pooled streams and the event between them, given back on every path
        int device; hipStream_t a = nullptr, b = nullptr; hipEvent_t ev = nullptr;
        explicit Streams(int d) : device(d) {
            a = take_stream(d, 0); b = take_stream(d, 0);
            HIPCHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        }
        ~Streams() {
            hipStreamSynchronize(a); hipStreamSynchronize(b);
            if (ev) hipEventDestroy(ev);
            give_stream(device, 0, a); give_stream(device, 0, b);
        }
    } st(device);
    DevBuf buf(n), res(n);
    // buf = 1.0, and every kernel used below has run once (a first launch may load its code, which would hold the host back by
    // more than the delay under test): all complete before anything below is issued
    HIPCHECK(p3d_fill_uniform(buf.p, n, 1.f, 1.f, 0, st.a));
    HIPCHECK(p3d_delay(1, st.a));
    HIPCHECK(hipStreamSynchronize(st.a));
    HIPCHECK(p3d_copy_strided(res.p, 4, buf.p, 4, n / 4, 4, st.b));
    HIPCHECK(hipStreamSynchronize(st.b));
    HIPCHECK(fill_now(res.p, 0, (size_t)n * 4, st.b));
    Perturb pt;
    pt.mode = mode; pt.streams[0] = st.a; pt.streams[1] = st.b;
    if (mode == 2) { pt.target = slow ? st.b : st.a; pt.delay_us = delay_us; }
    Perturb* const before = g_perturb;
    g_perturb = mode ? &pt : nullptr;
    try {
        Ctx ca, cb; ca.s = st.a; cb.s = st.b;
        launch(ca, "fill_uniform_kernel", 0, 4.0 * n, [&]() { return p3d_fill_uniform(buf.p, n, 2.f, 2.f, 0, ca.s); });
        HIPCHECK(ev_record(st.ev, st.a));
        if (with_wait) HIPCHECK(ev_wait(st.b, st.ev));
        launch(cb, "add_inplace_kernel", 0, 8.0 * n, [&]() { return p3d_copy_strided(res.p, 4, buf.p, 4, n / 4, 4, cb.s); });
        HIPCHECK(hipStreamSynchronize(st.a));
        HIPCHECK(hipStreamSynchronize(st.b));
    } catch (...) { g_perturb = before; throw; }
    g_perturb = before;
    res.get(out, n);
    API_END
}

int p3d_debug_conv_launch(int device, int kind, const float* in, int ld_in, int off_in, const int64_t xs[5], const float* w,
                          const int64_t ws[5], const int s[3], const float* bias, int accum, int f16, float* out, int ld_out, int off_out,
                          char* kernels, int kernels_cap, int* splits) {
    API_BEGIN
    HIPCHECK(hipSetDevice(device));
    if (!in || !xs || !w || !ws || !s || !out) throw P3dError("null argument");
    if (kind < 0 || kind > 2) throw P3dError("conv_launch: kind is 0 (forward), 1 (input gradient) or 2 (transposed forward)");
    const ConvProblem p = conv_problem(xs, ws, s, kind == 2);
    if (p.stem) throw P3dError("conv_launch: the stem shape has its own entry points");
    if (kind != 2 && ws[3] != p.Cin) throw P3dError("filter Cin mismatch");
    if (kind == 2 && accum) throw P3dError("conv_launch: a transposed conv's forward never accumulates");
    if (kind == 1 && bias) throw P3dError("conv_launch: an input gradient has no bias");
    const int ntap = (int)(ws[0] * ws[1] * ws[2]);
    if (f16 && (ntap != 1 || kind == 2)) throw P3dError("conv_launch: the fp16 option is for 1x1x1 convs, forward and input gradient");
    // gathered side / output side: (rows, channels)
    const int64_t rin = kind == 1 ? p.rows : p.rows_in, rout = kind == 1 ? p.rows_in : p.rows;
    const int cin = kind == 1 ? p.Cout : p.Cin, cout = kind == 1 ? p.Cin : p.Cout;
    check_slice("conv_launch (gathered side)", ld_in, off_in, cin);
    check_slice("conv_launch (output side)", ld_out, off_out, cout);
    DevBuf din(rin * ld_in, in), dw(prod5(ws), w), dout(rout * ld_out, out), db(cout, bias);
    ensure_zero_page();
    const float* bp = bias ? db.p : nullptr;
    std::vector<IgemmArgs> v = kind == 1 ? p.input_gradient(din.p + off_in, dw.p, dout.p + off_out, ld_in, ld_out, accum ? 1 : 0)
                                         : p.forward(din.p + off_in, dw.p, dout.p + off_out, bp, nullptr, nullptr, ld_in, ld_out, accum ? 1 : 0);
    if (f16) for (auto& a : v) a.f16 = 1;      // (conv(): set on the built launches)
    Ctx c;
    std::string names;
    traced_kernels([&]() { run_igemm_group(c, v, accum != 0, nullptr); }, names);
    // a single launch whose last round goes out K-sliced keeps its tile's name in the step's tables; say so here
    if (v.size() == 1 && p3d_igemm2_tail_split(v[0], p3d_igemm2_plan(v[0], 1))) names += "(tail)";
    put_string(names, kernels, kernels_cap);
    if (splits) {          // K-slices of the launches' plans (the names do not carry them): the smallest and the largest
        splits[0] = 1 << 30; splits[1] = 0;
        for (const IgemmArgs& a : v) {
            const P3dIgemmPlan pl = p3d_igemm2_plan(a, 1);
            const int sp = pl.stream_blocks > 0 || pl.splits < 1 ? 1 : pl.splits;
            splits[0] = std::min(splits[0], sp); splits[1] = std::max(splits[1], sp);
        }
        if (v.empty()) splits[0] = splits[1] = 0;
    }
    dout.get(out, rout * ld_out);
    API_END
}

int p3d_debug_wgrad_group(int device, int n, const float* const* x, const int* ldx, const int* offx, const int64_t* xs,
                          const float* const* dy, const int* lddy, const int* offdy, const int64_t* ws, const int* s, const int* transpose,
                          float* const* dw, float* const* dbias, int polite, int greedy, char* kernel, int kernel_cap, int* cuts,
                          int* info) {
    API_BEGIN
    HIPCHECK(hipSetDevice(device));
    if (!x || !ldx || !offx || !xs || !dy || !lddy || !offdy || !ws || !s || !transpose || !dw || !dbias || !cuts || !info)
        throw P3dError("null argument");
    if (n < 1 || n > P3D_WGRAD_GROUP) throw P3dError("wgrad_group: 1 to " + std::to_string(P3D_WGRAD_GROUP) + " problems");
    struct Bufs { std::unique_ptr<DevBuf> x, dy, dw, db; int64_t nw; int nb; };
    std::vector<Bufs> bufs((size_t)n);
    std::vector<WgradArgs> probs;
    ensure_zero_page();
    double fl = 0, by = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t* xsi = xs + 5 * i; const int64_t* wsi = ws + 5 * i;
        const ConvProblem p = conv_problem(xsi, wsi, s + 3 * i, transpose[i]);
        if (p.stem) throw P3dError("wgrad_group: the stem shape has its own entry points");
        if (!transpose[i] && wsi[3] != p.Cin) throw P3dError("filter Cin mismatch");
        if (transpose[i] && dbias[i]) throw P3dError("wgrad_group: a transposed conv's bias gradient is a column sum of its own");
        check_slice("wgrad_group (x)", ldx[i], offx[i], p.Cin);
        check_slice("wgrad_group (dy)", lddy[i], offdy[i], p.Cout);
        Bufs& b = bufs[(size_t)i];
        b.nw = prod5(wsi); b.nb = p.Cout;
        b.x.reset(new DevBuf(p.rows_in * ldx[i], x[i]));
        b.dy.reset(new DevBuf(p.rows * lddy[i], dy[i]));
        if (b.nw > 0 && !dw[i]) throw P3dError("null argument");
        b.dw.reset(new DevBuf(b.nw, dw[i]));
        if (dbias[i]) b.db.reset(new DevBuf(b.nb, dbias[i]));
        WgradArgs a = p.filter_gradient(b.x->p + offx[i], ldx[i], b.dy->p + offdy[i], lddy[i], b.dw->p, dbias[i] ? b.db->p : nullptr);
        a.zeros = g_zero_page;
        a.polite = polite ? 1 : 0; a.greedy = greedy ? 1 : 0;
        double f1, b1;
        wgrad_work(a, f1, b1);
        fl += f1; by += b1;
        probs.push_back(a);
    }
    info[1] = info[2] = 0;
    if (p3d_wgrad2_group_cuts(probs.data(), n, cuts, &info[0], &info[1], &info[2]) < 0) throw P3dError("wgrad_group: a problem the kernel does not take");
    const char* name = wgrad_group_name(probs);
    put_string(name, kernel, kernel_cap);
    Ctx c;
    launch_wgrad_group(c, probs, name, fl, by);
    for (int i = 0; i < n; ++i) {
        if (bufs[(size_t)i].nw > 0) bufs[(size_t)i].dw->get(dw[i], bufs[(size_t)i].nw);
        if (dbias[i]) bufs[(size_t)i].db->get(dbias[i], bufs[(size_t)i].nb);
    }
    API_END
}

// ---- fused-BatchNorm launches (test hooks, include/p3d_hip.h): the builders of conv() on host arrays --------------------------------
namespace {
// a host array that a launch may write: on the device for the launch, back in the caller's array afterwards (null: absent)
struct InOut {
    std::unique_ptr<DevBuf> d; float* host = nullptr; int64_t n = 0;
    void put(float* h, int64_t count) { host = h; n = count; if (h) d.reset(new DevBuf(count, h)); }
    float* p() const { return d ? d->p : nullptr; }
    void back() { if (d) d->get(host, n); }
};
std::unique_ptr<DevBuf> dev_copy(const float* h, int64_t n) { return std::unique_ptr<DevBuf>(h ? new DevBuf(n, h) : nullptr); }
void report_splits(const std::vector<IgemmArgs>& v, int* splits) {
    if (!splits) return;
    splits[0] = 1 << 30; splits[1] = 0;
    for (const IgemmArgs& a : v) {
        const P3dIgemmPlan pl = p3d_igemm2_plan(a, 1);
        const int sp = pl.stream_blocks > 0 || pl.splits < 1 ? 1 : pl.splits;
        splits[0] = std::min(splits[0], sp); splits[1] = std::max(splits[1], sp);
    }
    if (v.empty()) splits[0] = splits[1] = 0;
}
}  // namespace

int p3d_debug_fused_conv(int device, p3d_fused_conv* fc, char* kernels, int kernels_cap, int* splits) {
    API_BEGIN
    HIPCHECK(hipSetDevice(device));
    if (!fc || !fc->w || !fc->out) throw P3dError("null argument");
    if (fc->kind != 0 && fc->kind != 1) throw P3dError("fused_conv: kind is 0 (forward) or 1 (input gradient)");
    const ConvProblem p = conv_problem(fc->xshape, fc->wshape, fc->stride, 0);
    if (p.stem) throw P3dError("fused_conv: the stem shape has its own entry points");
    if (fc->wshape[3] != p.Cin) throw P3dError("filter Cin mismatch");
    const int ntap = (int)(fc->wshape[0] * fc->wshape[1] * fc->wshape[2]);
    if (fc->f16 && ntap != 1) throw P3dError("fused_conv: the fp16 option is for 1x1x1 convs");
    ensure_zero_page();
    DevBuf dw(prod5(fc->wshape), fc->w);
    Ctx c;
    std::string names;
    std::vector<IgemmArgs> v;
    fc->gpart_rows = 0;
    if (fc->kind == 0) {
        if (fc->at != P3D_AT_RELU1 && fc->at != P3D_AT_RELU2) throw P3dError("fused_conv: a forward launch has at = 1 (RELU1) or 2 (RELU2)");
        check_slice("fused_conv (output)", fc->ld_out, fc->off_out, p.Cout);
        std::unique_ptr<DevBuf> y[2], gamma[2], beta[2], part[2], db = dev_copy(fc->bias, p.Cout);
        InOut pub[2][6];
        FusedBn d[2];
        const float* yp[2] = {nullptr, nullptr};
        for (int q = 0; q < fc->at; ++q) {
            const p3d_fused_bn& b = fc->src[q];
            if (!b.y || !b.scale || !b.shift || !b.mean || !b.invstd) throw P3dError("null argument");
            check_slice("fused_conv (source)", b.ld, b.off, p.Cin);
            if (q == 1 && b.y == fc->src[0].y && b.ld == fc->src[0].ld) yp[1] = y[0]->p + b.off;      // two slices of ONE buffer
            else { y[q].reset(new DevBuf(p.rows_in * b.ld, b.y)); yp[q] = y[q]->p + b.off; }
            float* const arr[6] = {b.scale, b.shift, b.mean, b.invstd, b.moving_mean, b.moving_var};
            for (int j = 0; j < 6; ++j) pub[q][j].put(arr[j], p.Cin);
            d[q].C = p.Cin; d[q].rows = b.rows;
            d[q].scale = pub[q][0].p(); d[q].shift = pub[q][1].p(); d[q].mean = pub[q][2].p(); d[q].invstd = pub[q][3].p();
            d[q].moving_mean = pub[q][4].p(); d[q].moving_var = pub[q][5].p();
            d[q].update_moving = b.update_moving != 0;
            if (b.partials) {
                if (!b.gamma || !b.beta) throw P3dError("null argument");
                if (b.nparts < 1 || b.rows < 1) throw P3dError("fused_conv: partials need nparts >= 1 and rows >= 1");
                if (b.publish && b.update_moving && (!b.moving_mean || !b.moving_var)) throw P3dError("null argument");
                gamma[q] = dev_copy(b.gamma, p.Cin); beta[q] = dev_copy(b.beta, p.Cin);
                part[q] = dev_copy(b.partials, (int64_t)b.nparts * p.Cin * 2);
                d[q].gamma = gamma[q]->p; d[q].beta = beta[q]->p; d[q].part = part[q]->p; d[q].nparts = b.nparts;
                d[q].pub = b.publish ? 1 : 2;
            } else d[q].rows = 1;
        }
        v = p.forward(yp[0], dw.p, nullptr, db ? db->p : nullptr, nullptr, nullptr, fc->src[0].ld, fc->ld_out, 0);
        DevBuf dout(p.rows * fc->ld_out, fc->out);
        v[0].y = dout.p + fc->off_out;
        traced_kernels([&]() {
            bool fin[2] = {false, false};
            for (int q = 0; q < fc->at; ++q) fin[q] = fused_bn_prefinalize(c, d[q]);      // (conv(): ahead of the launch, on its stream)
            fused_forward_operand(v[0], fc->at, d[0], fin[0], yp[1], fc->src[1].ld, fc->at == P3D_AT_RELU2 ? &d[1] : nullptr, fin[1]);
            if (fc->f16) v[0].f16 = 1;
            run_igemm_group(c, v, false, nullptr);
        }, names);
        dout.get(fc->out, p.rows * fc->ld_out);
        for (int q = 0; q < fc->at; ++q) for (int j = 0; j < 6; ++j) pub[q][j].back();
    } else {
        if (!fc->g) throw P3dError("null argument");
        if (fc->bias) throw P3dError("fused_conv: an input gradient has no bias");
        if (fc->ngate < 0 || fc->ngate > 2) throw P3dError("fused_conv: 0, 1 or 2 gates");
        fused_gate_check(fc->stride, fc->ngate);
        check_slice("fused_conv (gradient)", fc->ld_g, fc->off_g, p.Cout);
        check_slice("fused_conv (raw result)", fc->ld_out, fc->off_out, p.Cin);
        DevBuf dg(p.rows * fc->ld_g, fc->g), dout(p.rows_in * fc->ld_out, fc->out);
        const int accum = fc->accum ? 1 : 0;
        v = p.input_gradient(dg.p + fc->off_g, dw.p, dout.p + fc->off_out, fc->ld_g, fc->ld_out, accum);
        if (fc->f16) for (auto& a : v) a.f16 = 1;
        // GRAD operand
        std::unique_ptr<DevBuf> gy, ggamma, gmean, ginv, gpart;
        InOut gout[3];
        FusedBnGrad gd;
        if (fc->grad) {
            const p3d_fused_bn_grad& b = fc->gbn;
            if (!b.y || !b.coef) throw P3dError("null argument");
            check_slice("fused_conv (BatchNorm input)", b.ld, b.off, p.Cout);
            gy.reset(new DevBuf(p.rows * b.ld, b.y));
            gout[0].put(b.coef, 3 * (int64_t)p.Cout); gout[1].put(b.dgamma, p.Cout); gout[2].put(b.dbeta, p.Cout);
            gd.C = p.Cout; gd.rows = 1; gd.coef = gout[0].p(); gd.dgamma = gout[1].p(); gd.dbeta = gout[2].p();
            if (b.partials) {
                if (!b.gamma || !b.mean || !b.invstd) throw P3dError("null argument");
                if (b.nparts < 1 || b.rows < 1) throw P3dError("fused_conv: partials need nparts >= 1 and rows >= 1");
                if (b.publish && (!b.dgamma || !b.dbeta)) throw P3dError("null argument");
                if (!b.publish && fused_needs_finalize(b.nparts)) throw P3dError("fused_conv: that many partials go through the finalize launch, which publishes");
                ggamma = dev_copy(b.gamma, p.Cout); gmean = dev_copy(b.mean, p.Cout); ginv = dev_copy(b.invstd, p.Cout);
                gpart = dev_copy(b.partials, (int64_t)b.nparts * p.Cout * 2);
                gd.gamma = ggamma->p; gd.mean = gmean->p; gd.invstd = ginv->p; gd.part = gpart->p; gd.nparts = b.nparts; gd.rows = b.rows;
            }
        }
        // gates
        std::unique_ptr<DevBuf> qy[2], qtab[2][4];
        InOut qout[2], qpart[2];
        BnGate gates[2];
        for (int q = 0; q < fc->ngate; ++q) {
            const p3d_fused_gate& b = fc->gate[q];
            if (!b.y || !b.scale || !b.shift || !b.mean || !b.invstd || !b.out || !b.part) throw P3dError("null argument");
            if (b.part_rows < 1) throw P3dError("fused_conv: a gate needs room for its partials");
            check_slice("fused_conv (gate input)", b.ld_y, b.off_y, p.Cin);
            check_slice("fused_conv (gated gradient)", b.ld_out, b.off_out, p.Cin);
            qy[q].reset(new DevBuf(p.rows_in * b.ld_y, b.y));
            const float* const tabs[4] = {b.scale, b.shift, b.mean, b.invstd};
            for (int j = 0; j < 4; ++j) qtab[q][j] = dev_copy(tabs[j], p.Cin);
            qout[q].put(b.out, p.rows_in * b.ld_out);
            qpart[q].put(b.part, (int64_t)b.part_rows * p.Cin * 2);
            memset(&gates[q], 0, sizeof(BnGate));
            gates[q].y = qy[q]->p + b.off_y; gates[q].ldy = b.ld_y;
            gates[q].scale = qtab[q][0]->p; gates[q].shift = qtab[q][1]->p; gates[q].mean = qtab[q][2]->p; gates[q].invstd = qtab[q][3]->p;
            gates[q].out = qout[q].p() + b.off_out; gates[q].ldo = b.ld_out;
            gates[q].part = qpart[q].p();
        }
        traced_kernels([&]() {
            if (fc->grad) {
                const bool fin = fc->gbn.partials ? fused_bn_grad_prefinalize(c, gd) : true;      // published coefficients: nothing to fold
                bool first = true;
                for (auto& a : v) { fused_grad_operand(a, gy->p + fc->gbn.off, fc->gbn.ld, gd, fin, first && fc->gbn.publish); first = false; }
            }
            if (fc->ngate) {
                const int mt = fused_gated_epilogue(v, fc->ngate, gates, fc->raw_store != 0, true);
                for (int q = 0; q < fc->ngate; ++q)
                    if (mt > fc->gate[q].part_rows) throw P3dError("gradient partials overflow their buffer");
                fc->gpart_rows = mt;
            }
            run_igemm_group(c, v, accum != 0, nullptr);
        }, names);
        dout.get(fc->out, p.rows_in * fc->ld_out);
        for (int j = 0; j < 3; ++j) gout[j].back();
        for (int q = 0; q < fc->ngate; ++q) { qout[q].back(); qpart[q].back(); }
    }
    put_string(names, kernels, kernels_cap);
    report_splits(v, splits);
    API_END
}

int p3d_debug_fused_wgrad(int device, int n, const float* const* x, const int* ldx, const int* offx, const int64_t* xs,
                          const float* const* dy, const int* lddy, const int* offdy, const int64_t* ws, const int* s,
                          const int* xt, const float* const* x2, const int* ldx2, const int* offx2, const float* const* xs1,
                          const float* const* xt1, const float* const* xs2, const float* const* xt2, const int* dyt,
                          const float* const* dy2, const int* lddy2, const int* offdy2, const float* const* dcoef,
                          float* const* dw, float* const* dbias, char* kernel, int kernel_cap, int* cuts, int* info) {
    API_BEGIN
    HIPCHECK(hipSetDevice(device));
    if (!x || !ldx || !offx || !xs || !dy || !lddy || !offdy || !ws || !s || !xt || !x2 || !ldx2 || !offx2 || !xs1 || !xt1 || !xs2 || !xt2 ||
        !dyt || !dy2 || !lddy2 || !offdy2 || !dcoef || !dw || !dbias || !cuts || !info)
        throw P3dError("null argument");
    if (n < 1 || n > P3D_WGRAD_GROUP) throw P3dError("fused_wgrad: 1 to " + std::to_string(P3D_WGRAD_GROUP) + " problems");
    struct Bufs { std::unique_ptr<DevBuf> x, x2, dy, dy2, s1, t1, s2, t2, coef, dw, db; int64_t nw; int nb; };
    std::vector<Bufs> bufs((size_t)n);
    std::vector<WgradArgs> probs;
    ensure_zero_page();
    double fl = 0, by = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t* xsi = xs + 5 * i; const int64_t* wsi = ws + 5 * i;
        const ConvProblem p = conv_problem(xsi, wsi, s + 3 * i, 0);
        if (p.stem) throw P3dError("fused_wgrad: the stem shape has its own entry points");
        if (wsi[3] != p.Cin) throw P3dError("filter Cin mismatch");
        if (!x[i] || !dy[i]) throw P3dError("null argument");
        check_slice("fused_wgrad (x)", ldx[i], offx[i], p.Cin);
        check_slice("fused_wgrad (dy)", lddy[i], offdy[i], p.Cout);
        Bufs& b = bufs[(size_t)i];
        b.nw = prod5(wsi); b.nb = p.Cout;
        b.x.reset(new DevBuf(p.rows_in * ldx[i], x[i]));
        b.dy.reset(new DevBuf(p.rows * lddy[i], dy[i]));
        if (b.nw > 0 && !dw[i]) throw P3dError("null argument");
        b.dw.reset(new DevBuf(b.nw, dw[i]));
        if (dbias[i]) b.db.reset(new DevBuf(b.nb, dbias[i]));
        WgradArgs a = p.filter_gradient(b.x->p + offx[i], ldx[i], b.dy->p + offdy[i], lddy[i], b.dw->p, dbias[i] ? b.db->p : nullptr);
        a.zeros = g_zero_page;
        if (xt[i]) {
            if (xt[i] != 1 && xt[i] != 2) throw P3dError("fused_wgrad: xt is 0, 1 or 2");
            if (!xs1[i] || !xt1[i]) throw P3dError("null argument");
            b.s1 = dev_copy(xs1[i], p.Cin); b.t1 = dev_copy(xt1[i], p.Cin);
            const float* x2p = nullptr;
            if (xt[i] == 2) {
                if (!x2[i] || !xs2[i] || !xt2[i]) throw P3dError("null argument");
                check_slice("fused_wgrad (x2)", ldx2[i], offx2[i], p.Cin);
                b.s2 = dev_copy(xs2[i], p.Cin); b.t2 = dev_copy(xt2[i], p.Cin);
                if (x2[i] == x[i] && ldx2[i] == ldx[i]) x2p = b.x->p + offx2[i];      // two slices of ONE buffer
                else { b.x2.reset(new DevBuf(p.rows_in * ldx2[i], x2[i])); x2p = b.x2->p + offx2[i]; }
            }
            fused_wgrad_x(a, xt[i], b.s1->p, b.t1->p, x2p, ldx2[i], b.s2 ? b.s2->p : nullptr, b.t2 ? b.t2->p : nullptr);
        }
        if (dyt[i]) {
            if (!dy2[i] || !dcoef[i]) throw P3dError("null argument");
            check_slice("fused_wgrad (dy2)", lddy2[i], offdy2[i], p.Cout);
            b.dy2.reset(new DevBuf(p.rows * lddy2[i], dy2[i]));
            b.coef = dev_copy(dcoef[i], 3 * (int64_t)p.Cout);
            fused_wgrad_dy(a, b.dy2->p + offdy2[i], lddy2[i], b.coef->p);
        }
        double f1, b1;
        wgrad_work(a, f1, b1);
        fl += f1; by += b1;
        probs.push_back(a);
    }
    info[1] = info[2] = 0;
    if (p3d_wgrad2_group_cuts(probs.data(), n, cuts, &info[0], &info[1], &info[2]) < 0) throw P3dError("fused_wgrad: a problem the kernel does not take");
    const char* name = wgrad_group_name(probs);
    put_string(name, kernel, kernel_cap);
    Ctx c;
    launch_wgrad_group(c, probs, name, fl, by);
    for (int i = 0; i < n; ++i) {
        if (bufs[(size_t)i].nw > 0) bufs[(size_t)i].dw->get(dw[i], bufs[(size_t)i].nw);
        if (dbias[i]) bufs[(size_t)i].db->get(dbias[i], bufs[(size_t)i].nb);
    }
    API_END
}

int p3d_debug_fused_reject(int device, int which, int* error, int* validator) {
    API_BEGIN
    if (!error || !validator) throw P3dError("null argument");
    if (which < 0 || which > 9) throw P3dError("fused_reject: cases 0 to 9");
    // Every pointer names real memory, on the device where there is one: a launch that a broken check lets through writes into
    // this page and nowhere else.  Without a device the checks under test, which run ahead of any HIP call, answer all the same.
    int ndev = 0;
    const bool dev = hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
    if (!dev) (void)hipGetLastError();
    static float host_page[16384];
    std::unique_ptr<DevBuf> page;
    float* b = host_page;
    if (dev) { HIPCHECK(hipSetDevice(device)); page.reset(new DevBuf(16384)); b = page->p; }
    const int64_t xs[5] = {1, 1, 2, 2, 8}, ws[5] = {1, 1, 1, 8, 8};
    const int st[3] = {1, 1, 1};
    const ConvProblem p = conv_problem(xs, ws, st, 0);
    float *x = b, *w = b + 1024, *y = b + 2048, *tab = b + 4096, *part = b + 8192, *zeros = b + 12288;
    *error = 0; *validator = 1;
    if (which <= 6) {
        IgemmArgs a = p.forward(x, w, y, nullptr)[0];
        a.zeros = zeros;
        FusedBn d;
        d.gamma = tab; d.beta = tab + 8; d.C = 8; d.scale = tab + 16; d.shift = tab + 24; d.mean = tab + 32; d.invstd = tab + 40;
        d.moving_mean = tab + 48; d.moving_var = tab + 56; d.part = part; d.rows = 4; d.pub = 2;
        FusedBnGrad gd;
        gd.gamma = tab; gd.mean = tab + 32; gd.invstd = tab + 40; gd.C = 8; gd.coef = tab + 64; gd.dgamma = tab + 96; gd.dbeta = tab + 104;
        gd.part = part; gd.rows = 4;
        if (which == 0 || which == 1) { d.nparts = which ? P3D_FOLD_MAX + 1 : 0; fused_forward_operand(a, P3D_AT_RELU1, d, false, nullptr, 0, nullptr, false); }
        if (which == 2 || which == 3) { a.wT = 1; gd.nparts = which == 3 ? P3D_FOLD_MAX + 1 : 0; fused_grad_operand(a, y, 8, gd, false, false); }
        if (which == 4) {
            BnGate g;
            memset(&g, 0, sizeof(g));
            g.y = x; g.ldy = 8; g.scale = tab + 16; g.shift = tab + 24; g.mean = tab + 32; g.invstd = tab + 40; g.out = y + 512; g.ldo = 8; g.part = part;
            std::vector<IgemmArgs> v{a};
            fused_gated_epilogue(v, 1, &g, false, false);
            a = v[0];
            a.statpart = part + 4096;
        }
        if (which == 5) { d.pub = 0; fused_forward_operand(a, P3D_AT_RELU1, d, false, nullptr, 0, nullptr, false); a.wT = 1; }
        if (which == 6) { d.pub = 0; fused_forward_operand(a, P3D_AT_RELU2, d, false, x, 10, &d, false); }
        P3dIgemmPlan pl;
        pl.bm = 64; pl.bn = 64; pl.splits = 1; pl.name = "igemm2_kernel<64,64>";
        *error = (int)p3d_launch_igemm2(a, pl, nullptr);
    } else {
        WgradArgs a = p.filter_gradient(x, 8, y, 8, w, nullptr);
        a.zeros = zeros;
        if (which == 7) { fused_wgrad_x(a, 1, tab + 16, tab + 24, nullptr, 0, nullptr, nullptr); a.pair = 1; }
        if (which == 8) fused_wgrad_x(a, 2, tab + 16, tab + 24, x, 10, tab + 16, tab + 24);
        if (which == 9) { fused_wgrad_dy(a, y, 8, tab + 64); a.pair = 1; }
        int cuts[1], ks = 0, tm = 0, tn = 0;
        *validator = p3d_wgrad2_group_cuts(&a, 1, cuts, &ks, &tm, &tn) < 0 ? 0 : 1;
        *error = (int)p3d_launch_wgrad2_group(&a, 1, nullptr);
    }
    if (dev) HIPCHECK(hipDeviceSynchronize());
    API_END
}

int p3d_debug_max_pool3d(int device, const float* x, int ldx, int offx, const int64_t xs[5], const int k[3], const int s[3], float* y,
                         int ldy, int offy) {
    API_BEGIN
    HIPCHECK(hipSetDevice(device));
    if (!x || !xs || !k || !s || !y) throw P3dError("null argument");
    check_slice("max_pool3d (x)", ldx, offx, (int)xs[4]);
    check_slice("max_pool3d (y)", ldy, offy, (int)xs[4]);
    max_pool3d_on_host_arrays(x, ldx, offx, xs, k, s, y, y, ldy, offy);
    API_END
}

int p3d_debug_max_pool3d_grad(int device, const float* x, int ldx, int offx, const int64_t xs[5], const int k[3], const int s[3],
                              const float* dyh, int ldy, int offy, int accumulate, float* dxh, const char** kernel) {
    API_BEGIN
    HIPCHECK(hipSetDevice(device));
    if (!x || !xs || !k || !s || !dyh || !dxh) throw P3dError("null argument");
    check_slice("max_pool3d_grad (x, dx)", ldx, offx, (int)xs[4]);
    check_slice("max_pool3d_grad (y, dy)", ldy, offy, (int)xs[4]);
    const char* const ran = max_pool3d_grad_on_host_arrays(x, ldx, offx, xs, k, s, dyh, ldy, offy, accumulate ? 1 : 0, dxh, dxh);
    if (kernel) *kernel = ran;
    API_END
}

int p3d_debug_bias_add_grad(int device, const float* dyh, int64_t rows, int channels, int ld, int off, float* dbias) {
    API_BEGIN
    if (!dyh || !dbias) throw P3dError("null argument");
    if (rows < 0 || channels < 1 || off < 0 || ld < off + channels) throw P3dError("bias_add_grad needs rows >= 0, channels >= 1 and offset + channels <= row length");
    HIPCHECK(hipSetDevice(device));
    bias_add_grad_on_host_arrays(dyh, rows, channels, ld, off, dbias, dbias);
    API_END
}

namespace {
// a device buffer whose every float is a NaN (all bits set) until a launch writes it
struct NanBuf : DevBuf {
    explicit NanBuf(int64_t n) : DevBuf(n) { HIPCHECK(fill_now(p, 0xFF, (size_t)(n > 0 ? n : 1) * 4, nullptr)); }
};
// the attention core on dense host operands, mode 1 = stored scores (AttnCore), 2 = the kernels that keep the scores on chip;
// nan_fill: every output and scratch buffer holds NaNs before the launches
void attention_core_on_host_arrays(const char* who, int device, int mode, bool nan_fill, int batch, int n_g, int n_f, int ch, const float* gh,
                                   const float* fh, const float* hh, float* o, const float* d_o, float* dg, float* df, float* dh) {
    const std::string w(who);
    if (!gh || !fh || !hh || !o) throw P3dError("null argument");
    if (mode != 1 && mode != 2) throw P3dError(w + ": mode is 1 (stored scores) or 2 (scores on chip)");
    if (mode == 2 && !p3d_flash_attn_ok(ch)) throw P3dError(w + ": ch must be 32, 64, 128 or 256");
    if (mode == 1 && (ch < 32 || ch % 32)) throw P3dError(w + ": the stored-score execution takes channel counts that are multiples of 32");
    if (batch < 1 || n_g < 1 || n_f < 1) throw P3dError(w + " needs at least one clip, query and key");
    if (d_o && (!dg || !df || !dh)) throw P3dError(w + ": the backward pass writes dg, df and dh");
    HIPCHECK(hipSetDevice(device));
    const int ci = ch / 8;
    const int64_t ng = (int64_t)batch * n_g, nf = (int64_t)batch * n_f;
    auto fresh = [&](int64_t n) { return std::unique_ptr<DevBuf>(nan_fill ? new NanBuf(n) : new DevBuf(n)); };
    DevBuf g(ng * ci, gh), f(nf * ci, fh), h(nf * ch, hh);
    std::unique_ptr<DevBuf> out = fresh(ng * ch), dout, gg, gf, gv;
    if (d_o) { dout.reset(new DevBuf(ng * ch, d_o)); gg = fresh(ng * ci); gf = fresh(nf * ci); gv = fresh(nf * ch); }
    if (mode == 2) {
        std::unique_ptr<DevBuf> lse = fresh(ng), dsum = fresh(ng);
        FlashAttnArgs a;
        memset(&a, 0, sizeof(a));
        a.B = batch; a.Ng = n_g; a.Nf = n_f; a.ch = ch;
        a.g = g.p; a.ldg = ci; a.f = f.p; a.ldf = ci; a.h = h.p; a.ldh = ch; a.o = out->p; a.ldo = ch; a.lse = lse->p;
        HIPCHECK(p3d_flash_attn_fwd(a, nullptr));
        out->get(o, ng * ch);
        if (d_o) {
            a.d_o = dout->p; a.lddo = ch; a.dsum = dsum->p;
            a.dg = gg->p; a.lddg = ci; a.df = gf->p; a.lddf = ci; a.dh = gv->p; a.lddh = ch;
            HIPCHECK(p3d_flash_attn_bwd(a, nullptr));
        }
    } else {
        AttnCore a;
        a.B = batch; a.Ng = n_g; a.Nf = n_f; a.ch = ch;
        // the queries of a clip as a lattice with every extent below 1024 (the GEMM kernels pack lattice coordinates)
        int rest = n_g;
        for (int* e : {&a.gW, &a.gH}) {
            int d = std::min(rest, 1023);
            while (rest % d) --d;
            *e = d; rest /= d;
        }
        a.gD = rest;
        if (a.gD > 1023) throw P3dError(w + ": n_g has no factorisation into three extents below 1024");
        const int64_t nfp = (int64_t)batch * a.Nfp();
        std::unique_ptr<DevBuf> sbuf = fresh(ng * a.Nfp()), dsbuf = fresh(ng * a.Nfp()), fpad, hpad, dfpad, dhpad;
        if (a.pad()) { fpad = fresh(nfp * ci); hpad = fresh(nfp * ch); dfpad = fresh(nfp * ci); dhpad = fresh(nfp * ch); }
        a.g = g.p; a.ldg = ci; a.f = f.p; a.h = h.p; a.o = out->p; a.ldo = ch;
        a.sbuf = sbuf->p; a.dsbuf = dsbuf->p;
        if (a.pad()) { a.fpad = fpad->p; a.hpad = hpad->p; a.dfpad = dfpad->p; a.dhpad = dhpad->p; }
        ensure_zero_page();
        Ctx c;
        a.forward(c);
        out->get(o, ng * ch);
        if (d_o) {
            a.d_o = dout->p; a.dg = gg->p; a.df = gf->p; a.dh = gv->p;
            a.backward(c);
        }
    }
    if (d_o) { gg->get(dg, ng * ci); gf->get(df, nf * ci); gv->get(dh, nf * ch); }
}
}  // namespace

int p3d_op_attention_core(int device, int batch, int n_g, int n_f, int ch, const float* gh, const float* fh, const float* hh,
                          float* o, const float* d_o, float* dg, float* df, float* dh) {
    API_BEGIN
    attention_core_on_host_arrays("attention_core", device, 2, false, batch, n_g, n_f, ch, gh, fh, hh, o, d_o, dg, df, dh);
    API_END
}

int p3d_debug_attention_core(int device, int mode, int batch, int n_g, int n_f, int ch, const float* gh, const float* fh, const float* hh,
                             float* o, const float* d_o, float* dg, float* df, float* dh) {
    API_BEGIN
    attention_core_on_host_arrays("debug_attention_core", device, mode, true, batch, n_g, n_f, ch, gh, fh, hh, o, d_o, dg, df, dh);
    API_END
}

int p3d_debug_attention_splits(int batch, int n_g, int n_f, int ch, int* splits) {
    API_BEGIN
    if (!splits) throw P3dError("null argument");
    if (batch < 1 || n_g < 1 || n_f < 1 || ch < 32 || ch % 32) throw P3dError("debug_attention_splits: bad shape");
    // host only: the plans are a function of the shapes (AttnCore::splits never reads an operand)
    AttnCore a;
    a.B = batch; a.Ng = n_g; a.Nf = n_f; a.ch = ch; a.gW = n_g; a.ldg = ch / 8; a.ldo = ch;
    for (int k = 0; k < 4; ++k) splits[k] = a.splits(k);
    API_END
}

int p3d_debug_softmax_rows(int device, int backward, int64_t rows, int cols, int ld, float* s, float* d, int guard_rows) {
    API_BEGIN
    if (!s || (backward && !d)) throw P3dError("null argument");
    if (rows < 1 || cols < 1 || ld < cols || guard_rows < 0) throw P3dError("debug_softmax_rows needs rows >= 1, 1 <= cols <= ld and guard_rows >= 0");
    HIPCHECK(hipSetDevice(device));
    const int64_t n = (rows + guard_rows) * ld;
    DevBuf ds(n, s);
    if (!backward) {
        HIPCHECK(p3d_softmax_rows(ds.p, (long long)rows, cols, ld, nullptr));
        ds.get(s, n);
    } else {
        DevBuf dd(n, d);
        HIPCHECK(p3d_softmax_rows_bwd(ds.p, dd.p, (long long)rows, cols, ld, nullptr));
        dd.get(d, n);
    }
    API_END
}

int p3d_debug_attn_mix(int device, int64_t M, int C, const float* r, int ldr, int offr, const float* x, int ldx, int offx, float gamma,
                       float drop_rate, uint64_t seed, int seed_dev, float* z, int ldz, int offz, const float* dz, int accx, float* dr,
                       float* dx, float* dgamma) {
    API_BEGIN
    if (!r || !x || !z) throw P3dError("null argument");
    if (dz && (!dr || !dx || !dgamma)) throw P3dError("debug_attn_mix: the backward pass writes dr, dx and dgamma");
    if (M < 1) throw P3dError("debug_attn_mix needs at least one row");
    if (!(drop_rate >= 0.f && drop_rate < 1.f)) throw P3dError("debug_attn_mix: drop_rate in [0, 1)");
    check_slice("debug_attn_mix (r, dr)", ldr, offr, C);
    check_slice("debug_attn_mix (x, dx)", ldx, offx, C);
    check_slice("debug_attn_mix (z, dz)", ldz, offz, C);
    HIPCHECK(hipSetDevice(device));
    DevBuf dr_in(M * ldr, r), dx_in(M * ldx, x), dzz(M * ldz, z), dgm(1, &gamma);
    DevBuf dseed(2);
    HIPCHECK(copy_now(dseed.p, &seed, sizeof(seed), hipMemcpyHostToDevice, nullptr));
    Ctx c;         // (attn_run: the block's dropout, with the step's seed as an argument or in device memory)
    c.training = true; c.drop = drop_rate;
    if (seed_dev) c.seed_dev = reinterpret_cast<const unsigned long long*>(dseed.p); else c.seed = seed;
    auto args = [&](const float* g_z, float* g_r, float* g_x, float* g_gm) {
        return attn_mix_args(M, C, dr_in.p + offr, ldr, dx_in.p + offx, ldx, dgm.p, dzz.p + offz, ldz, g_z, g_r, g_x, accx ? 1 : 0, g_gm, c, true);
    };
    attn_mix_forward(c, args(nullptr, nullptr, nullptr, nullptr));
    dzz.get(z, M * ldz);
    if (dz) {
        DevBuf g_z(M * ldz, dz), g_r(M * ldr, dr), g_x(M * ldx, dx), g_gm(1, dgamma);
        attn_mix_backward(c, args(g_z.p + offz, g_r.p + offr, g_x.p + offx, g_gm.p));      // (part and counter: the launcher's, from the stream's scratch)
        g_r.get(dr, M * ldr); g_x.get(dx, M * ldx); g_gm.get(dgamma, 1);
    }
    API_END
}

int p3d_shutdown(void) {
    API_BEGIN
    if (g_live_handles.load() > 0)
        throw P3dError("p3d_shutdown with " + std::to_string(g_live_handles.load()) + " live handle(s): destroy them first (their scratch and captured graphs name the pools this call frees)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return 0;
    hipDeviceSynchronize();
    destroy_pooled_streams();
    p3d_release_scratch();
    if (g_zero_page) { hipFree((void*)g_zero_page); g_zero_page = nullptr; }
    API_END
}

}  // extern "C"
