// part of net.hip (members of p3d_handle): the three settings of the read-out that the handle only keeps -- smoothing and
// normalisation, histogram matching, and the evaluation pass's KL divergence / information gain.  Their stages are issued by
// net_readout.inc; no step, launch list or captured graph ever names anything here.
    // ---- smoothing and normalisation of output maps (p3d_set_postprocess) ------------------------------
    // Off by default, and off nothing here runs.  The setting is three numbers: the stage itself (postprocess.hip) is issued by
    // the two users of the handle's prediction, p3d_eval_last_frames and p3d_pred_maps_u8 (net_readout.inc: post_sequence), with
    // scratch from the stream pool at first use.
    struct PostCfg {
        bool on = false;
        p3d_postprocess cfg{0.f, 0, P3D_NORM_NONE};
        // the effective radius (include/p3d_hip.h, RADIUS); throws on a setting the header refuses
        static int radius(const p3d_postprocess& c) {
            if (!std::isfinite(c.sigma) || c.sigma < 0.f) throw P3dError("postprocess: sigma must be finite and >= 0");
            if (c.radius < 0 || c.radius > P3D_BLUR_MAX_RADIUS) throw P3dError("postprocess: radius must be in [0, " + std::to_string(P3D_BLUR_MAX_RADIUS) + "]");
            if (c.radius > 0 && c.sigma == 0.f) throw P3dError("postprocess: a radius needs sigma > 0");
            if (c.norm != P3D_NORM_NONE && c.norm != P3D_NORM_MAX && c.norm != P3D_NORM_RANGE) throw P3dError("postprocess: unknown norm " + std::to_string(c.norm));
            if (c.radius > 0 || c.sigma == 0.f) return c.radius;
            const double k = std::rint(8.0 * (double)c.sigma + 1.0);
            if (k > 2.0 * P3D_BLUR_MAX_RADIUS + 1.0)
                throw P3dError("postprocess: sigma asks for a radius above " + std::to_string(P3D_BLUR_MAX_RADIUS) + "; give a radius");
            return ((int)k | 1) / 2;
        }
        static bool neutral(const p3d_postprocess& c) { return c.sigma == 0.f && c.radius == 0 && c.norm == P3D_NORM_NONE; }
        // the 2r + 1 weights (include/p3d_hip.h, TAPS), r >= 1
        static std::vector<float> taps(float sigma, int r) {
#pragma clang fp contract(off)
            std::vector<double> e((size_t)(2 * r + 1));
            const double s2 = 2.0 * ((double)sigma * (double)sigma);
            double S = 0.0;
            for (int k = 0; k <= 2 * r; ++k) {
                const double d = (double)(k - r);
                e[(size_t)k] = std::exp(-(d * d) / s2);
                S += e[(size_t)k];
            }
            std::vector<float> w(e.size());
            for (size_t k = 0; k < e.size(); ++k) w[k] = (float)(e[k] / S);
            return w;
        }
    } post;
    void set_postprocess(const p3d_postprocess* c) {
        const p3d_postprocess neutral{0.f, 0, P3D_NORM_NONE};
        const p3d_postprocess want = c ? *c : neutral;
        PostCfg::radius(want);                     // refuses before anything changes
        post.on = !PostCfg::neutral(want);
        post.cfg = post.on ? want : neutral;
    }

    // ---- histogram matching of output maps (p3d_set_hist_match; hist_match.hip) ---------------------------
    // Off by default, and off nothing here runs.  The setting is a mode, a bin count and (P3D_MATCH_TABLE) a copy of the caller's
    // table; the stage is issued by post_sequence (net_readout.inc) between the blur and the normalisation, with scratch from the
    // stream pool at first use.
    struct MatchCfg {
        int mode = P3D_MATCH_OFF, nb = 256;
        std::vector<double> cdf, centres;      // P3D_MATCH_TABLE: nt entries each
        bool on() const { return mode != P3D_MATCH_OFF; }
        static void bins(const char* what, int nb) {
            if (nb < 2 || nb > P3D_HIST_MAX_BINS)
                throw P3dError(std::string(what) + ": nbins must be in [2, " + std::to_string(P3D_HIST_MAX_BINS) + "], not " + std::to_string(nb));
        }
        // a supplied table as the header asks for it: 2 <= nt <= P3D_HIST_MAX_BINS, finite, non-decreasing (n_tables of them)
        static void table(const char* what, const double* cdf, const double* centres, int nt, int n_tables = 1) {
            if (nt < 2 || nt > P3D_HIST_MAX_BINS)
                throw P3dError(std::string(what) + ": nt must be in [2, " + std::to_string(P3D_HIST_MAX_BINS) + "], not " + std::to_string(nt));
            if (!cdf || !centres) throw P3dError(std::string(what) + ": a table needs cdf and centres");
            for (int t = 0; t < n_tables; ++t)
                for (int k = 0; k < nt; ++k) {
                    const double *a = cdf + (size_t)t * nt, *b = centres + (size_t)t * nt;
                    if (!std::isfinite(a[k]) || !std::isfinite(b[k])) throw P3dError(std::string(what) + ": the table must be finite (entry " + std::to_string(k) + ")");
                    if (k > 0 && (a[k] < a[k - 1] || b[k] < b[k - 1]))
                        throw P3dError(std::string(what) + ": the table must be non-decreasing (entry " + std::to_string(k) + ")");
                }
        }
        // what a p3d_hist_match asks for; throws on a setting the header refuses
        static MatchCfg parse(const p3d_hist_match* c) {
            MatchCfg m;
            if (!c || c->mode == P3D_MATCH_OFF) return m;
            if (c->mode != P3D_MATCH_TABLE && c->mode != P3D_MATCH_DENSITY) throw P3dError("hist_match: unknown mode " + std::to_string(c->mode));
            bins("hist_match", c->nbins);
            m.mode = c->mode; m.nb = c->nbins;
            if (c->mode == P3D_MATCH_TABLE) {
                table("hist_match", c->cdf, c->centres, c->nt);
                m.cdf.assign(c->cdf, c->cdf + c->nt);
                m.centres.assign(c->centres, c->centres + c->nt);
            }
            return m;
        }
    } match;
    void set_hist_match(const p3d_hist_match* c) { match = MatchCfg::parse(c); }      // (parsed first: a refusal changes nothing)

    // ---- KL divergence and information gain of the evaluation pass (p3d_set_eval_extra; metrics_full.hip) ----
    // Off by default, and off nothing here runs or exists.  The values of the last p3d_eval_last_frames stay on the host until
    // p3d_last_eval_extra.
    enum { EXTRA_NONE = 0, EXTRA_HAVE = 1, EXTRA_SHAPE = 2 };
    struct Extra {
        int flags = 0, H = 0, W = 0;
        DevMem<float> base; DevMem<double> bstat;      // the baseline [H * W] and its three statistics
        std::vector<float> base_host;                  // p3d_get_eval_extra hands the baseline back
        std::vector<double> last;                      // [B][2] of the last evaluation
        int state = EXTRA_NONE, eval_H = 0, eval_W = 0;
        // what the header asks of a setting; throws before anything changes
        static void check(int flags, const float* baseline, int H, int W) {
            if (flags & ~(P3D_EVAL_KLDIV | P3D_EVAL_INFO_GAIN)) throw P3dError("eval_extra: unknown flags " + std::to_string(flags));
            const bool ig = (flags & P3D_EVAL_INFO_GAIN) != 0;
            if (ig != (baseline != nullptr)) throw P3dError(ig ? "eval_extra: P3D_EVAL_INFO_GAIN needs a baseline" : "eval_extra: a baseline is given without P3D_EVAL_INFO_GAIN");
            if (!ig) return;
            if (H < 1 || W < 1 || (long long)H * W > INT32_MAX / 2) throw P3dError("eval_extra: the baseline is H x W floats, 1 <= H * W <= 2^30");
            const size_t n = (size_t)H * W;
            bool varies = false;
            for (size_t i = 0; i < n; ++i) {
                if (!std::isfinite(baseline[i])) throw P3dError("eval_extra: the baseline must be finite (element " + std::to_string(i) + ")");
                varies = varies || baseline[i] != baseline[0];
            }
            if (!varies) throw P3dError("eval_extra: the baseline must not be constant");
        }
        // a baseline on the device with its statistics, one launch on stream s (synchronised on return): base [H * W], bstat [3]
        static void upload(const float* baseline, int H, int W, float* base, double* bstat, hipStream_t s,
                           hipMemcpyKind kind = hipMemcpyHostToDevice) {
            const long long N = (long long)H * W;
            P3dFullStats3 q;
            q.maps = base; q.n_pix = N; q.n_maps = 1; q.nblk = p3d_full_blocks(N); q.out = bstat;
            DevMem<double> part((size_t)q.nblk * P3D_FULL_STATS3_PARTS, "eval_extra: no device memory for the baseline's partial sums");
            DevMem<unsigned> counter(1, "eval_extra: no device memory for the baseline's counter");
            q.part = part; q.counter = counter;
            HIPCHECK(copy_now(base, baseline, (size_t)N * sizeof(float), kind, s));
            HIPCHECK(fill_now(q.counter, 0, sizeof(unsigned), s));
            HIPCHECK(p3d_full_stats3(q, s));
            HIPCHECK(hipStreamSynchronize(s));
        }
        // flags with a baseline of H x W floats from `src` (host, or device under `kind`); null: no baseline
        static Extra make(int flags, const float* src, int H, int W, hipStream_t s, hipMemcpyKind kind = hipMemcpyHostToDevice) {
            Extra x;
            x.flags = flags;
            if (!src) return x;
            x.H = H; x.W = W;
            x.base = DevMem<float>((size_t)H * W, "eval_extra: no device memory for the baseline");
            x.bstat = DevMem<double>(3, "eval_extra: no device memory for the baseline's statistics");
            upload(src, H, W, x.base, x.bstat, s, kind);
            x.base_host.resize((size_t)H * W);
            if (kind == hipMemcpyHostToDevice) std::copy(src, src + (size_t)H * W, x.base_host.begin());
            else HIPCHECK(copy_now(x.base_host.data(), x.base, x.base_host.size() * sizeof(float), hipMemcpyDeviceToHost, s));
            return x;
        }
    } extra;
    // (the new setting first: a failure changes nothing)
    void set_eval_extra(int flags, const float* baseline, int H, int W) {
        Extra::check(flags, baseline, H, W);
        extra = Extra::make(flags, baseline, H, W, stream);
    }
    // p3d_set_eval_extra_prior: set_eval_extra with the handle's prior as the baseline, copied device to device; its statistics
    // come from the same one launch
    void set_eval_extra_prior(int flags) {
        if (flags & ~(P3D_EVAL_KLDIV | P3D_EVAL_INFO_GAIN)) throw P3dError("eval_extra: unknown flags " + std::to_string(flags));
        if (!(flags & P3D_EVAL_INFO_GAIN)) throw P3dError("eval_extra: a baseline is given without P3D_EVAL_INFO_GAIN");
        if (!prior.map) throw P3dError("eval_extra: the handle has no prior (p3d_prior_finish or p3d_set_prior_map)");
        extra = Extra::make(flags, prior.map, prior.H, prior.W, stream, hipMemcpyDeviceToDevice);
    }
