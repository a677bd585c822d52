// part of net.hip (members of p3d_handle): fixation priors (p3d_prior_*, p3d_set_prior_map, p3d_set_prior_stage; prior.hip).
// Nothing exists before p3d_prior_open or p3d_set_prior_map, and off nothing here runs.  No step, launch list or captured graph
// names the accumulator or the map.  The stage is issued by post_sequence (net_readout.inc) after the blur; the operations that
// need that sequence (finish) live in net_readout.inc.
    // the accumulator: uint32 counts, the underflow flag, a staging buffer for uploaded maps.  p3d_prior_close assigns a fresh one
    struct PriorAcc {
        bool is_open = false;
        int kind = P3D_PRIOR_FIXATIONS, H = 0, W = 0;
        int64_t n_maps = 0;
        DevMem<unsigned> count, flag;
        DevMem<unsigned char> staging;      // only grows
        void need_open(const char* what) const {
            if (!is_open) throw P3dError(std::string(what) + ": no accumulator is open (p3d_prior_open)");
        }
    } prior_acc;
    // the finished map with its stage; ms: the count launches of the last p3d_prior_add, the last p3d_prior_finish's launches
    struct PriorMap {
        DevMem<float> map; int H = 0, W = 0;
        int mode = P3D_PRIOR_OFF; float a = 0.f;
        double ms[2] = {0.0, 0.0};
        void take(DevMem<float>&& dev, int H_, int W_) {
            map = std::move(dev); H = map ? H_ : 0; W = map ? W_ : 0;
        }
        // a prior as the header asks for it: finite, not constant, 1 <= H * W <= 2^30
        static void check(const float* map, int H, int W) {
            if (!map) throw P3dError("null argument");
            if (H < 1 || W < 1 || (long long)H * W > INT32_MAX / 2) throw P3dError("prior: the map is H x W floats, 1 <= H * W <= 2^30");
            const size_t n = (size_t)H * W;
            bool varies = false;
            for (size_t i = 0; i < n; ++i) {
                if (!std::isfinite(map[i])) throw P3dError("prior: the map must be finite (element " + std::to_string(i) + ")");
                varies = varies || map[i] != map[0];
            }
            if (!varies) throw P3dError("prior: the map must not be constant");
        }
        static void stage_check(int mode, float a) {
            if (mode != P3D_PRIOR_OFF && mode != P3D_PRIOR_MUL && mode != P3D_PRIOR_MIX) throw P3dError("prior_stage: unknown mode " + std::to_string(mode));
            if (mode != P3D_PRIOR_OFF && !(a >= 0.f && a <= 1.f)) throw P3dError("prior_stage: the weight must be in [0, 1]");
        }
    } prior;
    void prior_open(int H, int W, int kind) {
        if (kind != P3D_PRIOR_FIXATIONS && kind != P3D_PRIOR_BYTES) throw P3dError("prior: kind " + std::to_string(kind) + " is neither P3D_PRIOR_FIXATIONS (0) nor P3D_PRIOR_BYTES (1)");
        if (H < 1 || W < 1 || (long long)H * W > INT32_MAX / 2) throw P3dError("prior: maps are H x W bytes, 1 <= H * W <= 2^30");
        PriorAcc acc;                          // the new accumulator first: a failure changes nothing
        acc.count = DevMem<unsigned>((size_t)H * W, "prior_open: no device memory for the counts");
        acc.flag = DevMem<unsigned>(1, "prior_open: no device memory for the underflow flag");
        HIPCHECK(fill_now(acc.count, 0, (size_t)H * W * sizeof(unsigned), stream));
        HIPCHECK(fill_now(acc.flag, 0, sizeof(unsigned), stream));
        acc.is_open = true; acc.kind = kind; acc.H = H; acc.W = W;
        prior_acc = std::move(acc);
    }
    bool prior_underflowed() {
        unsigned f = 0;
        HIPCHECK(copy_now(&f, prior_acc.flag, sizeof(f), hipMemcpyDeviceToHost, stream));
        return f != 0;
    }
    // maps [n][H][W] from the host, in uploads of at most 256 MB; sign +1 adds, -1 takes maps out again
    void prior_add(const unsigned char* maps, int64_t n, int sign) {
        prior_acc.need_open("prior_add");
        if (!maps) throw P3dError("null argument");
        if (sign != 1 && sign != -1) throw P3dError("prior_add: sign must be +1 or -1, not " + std::to_string(sign));
        if (n < 1) throw P3dError("prior_add: at least one map");
        if (sign > 0 && (n > P3D_PRIOR_MAX_MAPS || prior_acc.n_maps + n > P3D_PRIOR_MAX_MAPS))
            throw P3dError("prior_add: " + std::to_string(prior_acc.n_maps) + " + " + std::to_string(n) + " maps exceed P3D_PRIOR_MAX_MAPS = " + std::to_string((long long)P3D_PRIOR_MAX_MAPS));
        if (sign < 0 && n > prior_acc.n_maps)
            throw P3dError("prior_add: " + std::to_string(n) + " maps cannot leave an accumulator of " + std::to_string(prior_acc.n_maps));
        const size_t N = (size_t)prior_acc.H * prior_acc.W;
        const int64_t per = std::max<int64_t>(1, (int64_t)(((size_t)256 << 20) / N));
        prior_acc.staging.grow((size_t)std::min(n, per) * N, "prior_add: no device memory for the staging buffer");      // (every earlier call ended synchronised)
        StageTimer tm(true, 2);
        double ms = 0.0;
        for (int64_t done = 0; done < n; done += per) {
            const int64_t cn = std::min(per, n - done);
            PriorCountArgs a;
            a.maps = prior_acc.staging; a.n = cn; a.n_pix = (long long)N; a.kind = prior_acc.kind; a.sign = sign; a.count = prior_acc.count; a.flag = prior_acc.flag;
            HIPCHECK(copy_now(prior_acc.staging, maps + (size_t)done * N, (size_t)cn * N, hipMemcpyHostToDevice, stream));
            tm.mark(0, stream);
            HIPCHECK(p3d_prior_count_launch(a, stream));
            tm.mark(1, stream);
            HIPCHECK(hipStreamSynchronize(stream));
            ms += tm.ms(0);
            prior_acc.n_maps += sign * cn;
        }
        prior.ms[0] = ms;
    }
    void set_prior_map(const float* map, int H, int W) {
        if (!map) {                            // dropped; a stage that is on refuses when it next runs
            prior.take(DevMem<float>(), 0, 0);
            return;
        }
        PriorMap::check(map, H, W);
        DevMem<float> p((size_t)H * W, "set_prior_map: no device memory for the map");
        HIPCHECK(copy_now(p, map, (size_t)H * W * sizeof(float), hipMemcpyHostToDevice, stream));
        prior.take(std::move(p), H, W);
    }
    void set_prior_stage(int mode, float a) {
        PriorMap::stage_check(mode, a);
        if (mode != P3D_PRIOR_OFF && !prior.map) throw P3dError("prior_stage: the handle has no prior (p3d_prior_finish or p3d_set_prior_map)");
        prior.mode = mode; prior.a = mode != P3D_PRIOR_OFF ? a : 0.f;
    }
