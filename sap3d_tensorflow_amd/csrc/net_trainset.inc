// part of net.hip (members of p3d_handle): the resident training set (p3d_trainset_*; trainset.hip).  Nothing exists before the
// first p3d_trainset_open and nothing here runs while no set is open; no step, launch list or captured graph names the stores.
// The gather writes the staged x_in, d_y and d_fix, whose addresses never move, as the uploads do; d_fix is allocated by the first
// gather that writes it, as by the first p3d_upload_fixations.  The host keeps which frames were put, per tensor.  Every entry
// point ends synchronised, so the next call may overwrite the host table.
    // p3d_trainset_close assigns a fresh one; a p3d_trainset_open on an open set keeps the stores that are large enough
    struct TrainSet {
        bool is_open = false;
        int format = P3D_TRAINSET_FRAMES_U8, flags = 0;
        float mean[3] = {0.f, 0.f, 0.f};
        std::vector<int> frames;                 // F_v
        std::vector<int64_t> base;               // base[v] = F_0 + .. + F_{v-1}; [V + 1], the last entry the total
        DevMem<unsigned char> fr, den, fix;      // the three stores, in bytes (fr: bytes or floats, by `format`)
        DevMem<unsigned char> u8;                // staging of the puts that run a kernel; only grows
        DevMem<int> d_first;                     // the per-call table, [B]
        std::vector<int> first;
        std::vector<unsigned char> put[3];       // frames, density, fixations: [total]
        EventSet<2> ev;                          // around the last stage's launch (p3d_trainset_last_ms)
        bool timed = false;
        int64_t total() const { return base.empty() ? 0 : base.back(); }
        bool has_fix() const { return (flags & P3D_TRAINSET_FIXATIONS) != 0; }
        static const char* unput(int t) { return t == 0 ? ", which was never put" : t == 1 ? ", whose density map was never put" : ", whose fixation map was never put"; }

        // The global first frame of every clip of a stage, from host state alone (no HIP call): validates as the header says -- the
        // message names the first offending clip or frame.  put[t] (or null: the tensor is not written by the call) has one flag per
        // frame of the concatenation.
        static std::vector<int> plan(const char* who, const std::vector<int>& frames, const std::vector<int64_t>& base, int T, int B,
                                              const int* video, const int* start, int n, const unsigned char* const put[3]) {
            if (!video || !start) throw P3dError("null argument");
            if (n != B) throw P3dError(std::string(who) + ": " + std::to_string(n) + " clips, the batch is " + std::to_string(B));
            const int V = (int)frames.size();
            std::vector<int> first((size_t)B, 0);
            for (int k = 0; k < n; ++k) {
                const int v = video[k];
                if (v < 0 || v >= V)
                    throw P3dError(std::string(who) + ": clip " + std::to_string(k) + " names video " + std::to_string(v) + ", outside [0, " + std::to_string(V) + ")");
                const std::string c = std::string(who) + ": clip " + std::to_string(k) + " (video " + std::to_string(v) + ") starts at " + std::to_string(start[k]);
                if (start[k] < 0 || start[k] > frames[(size_t)v] - T)
                    throw P3dError(c + ", outside [0, F - T = " + std::to_string(frames[(size_t)v] - T) + "]");
                const int64_t f0 = base[(size_t)v] + start[k];
                for (int t = 0; t < 3; ++t)
                    for (int i = 0; put[t] && i < T; ++i)
                        if (!put[t][(size_t)(f0 + i)])
                            throw P3dError(c + " and holds frame " + std::to_string(start[k] + i) + unput(t));
                first[(size_t)k] = (int)f0;
            }
            return first;
        }

        void need_open(const char* who) const {
            if (!is_open) throw P3dError(std::string(who) + ": no training set is open (p3d_trainset_open)");
        }
        // frames first .. first + n - 1 of video v -> the first one's index in the concatenation
        int64_t range(const char* who, int v, int first, int n) const {
            if (v < 0 || v >= (int)frames.size())
                throw P3dError(std::string(who) + ": video " + std::to_string(v) + " is outside [0, " + std::to_string(frames.size()) + ")");
            if (n < 1 || first < 0 || first > frames[(size_t)v] - n)
                throw P3dError(std::string(who) + ": frames " + std::to_string(first) + " .. " + std::to_string((int64_t)first + n - 1) +
                               " are outside video " + std::to_string(v) + "'s [0, " + std::to_string(frames[(size_t)v]) + ")");
            return base[(size_t)v] + first;
        }
        void mark(int t, int64_t at, int n) { std::fill(put[t].begin() + at, put[t].begin() + at + n, (unsigned char)1); }
    } trainset;
    int64_t ts_hw() const { return (int64_t)x_in->H * x_in->W; }
    size_t ts_frame_bytes() const { return (size_t)ts_hw() * 3 * (trainset.format == P3D_TRAINSET_FRAMES_F32 ? 4 : 1); }

    void trainset_open(int n_videos, const int* frames, int format, int flags, const float mean_rgb[3]) {
        if (format != P3D_TRAINSET_FRAMES_U8 && format != P3D_TRAINSET_FRAMES_F32)
            throw P3dError("trainset_open: frame format " + std::to_string(format) + " is neither P3D_TRAINSET_FRAMES_U8 (0) nor P3D_TRAINSET_FRAMES_F32 (1)");
        if (flags & ~P3D_TRAINSET_FIXATIONS) throw P3dError("trainset_open: unknown flags " + std::to_string(flags));
        if (n_videos < 1) throw P3dError("trainset_open: needs at least one video");
        for (int c = 0; c < 3; ++c) if (!std::isfinite(mean_rgb[c])) throw P3dError("trainset_open: the channel means must be finite");
        std::vector<int64_t> base((size_t)n_videos + 1, 0);
        for (int v = 0; v < n_videos; ++v) {
            if (frames[v] < 1) throw P3dError("trainset_open: video " + std::to_string(v) + " has " + std::to_string(frames[v]) + " frames");
            base[(size_t)v + 1] = base[(size_t)v] + frames[v];
            if (base[(size_t)v + 1] > (int64_t)INT32_MAX) throw P3dError("trainset_open: more than 2^31 - 1 frames");
        }
        const int64_t total = base.back();
        const bool want_fix = (flags & P3D_TRAINSET_FIXATIONS) != 0;
        const size_t fb = (size_t)total * (size_t)ts_hw() * 3 * (format == P3D_TRAINSET_FRAMES_F32 ? 4 : 1), db = (size_t)total * (size_t)ts_hw();
        sync_streams();
        // the new stores first: a failed allocation changes nothing.  A store that is large enough stays
        const std::string what = "trainset_open: no device memory for " + std::to_string(total) + " frames";
        DevMem<unsigned char> nf, nd, nx;
        if (fb > trainset.fr.n) nf = DevMem<unsigned char>(fb, what);
        if (db > trainset.den.n) nd = DevMem<unsigned char>(db, what);
        if (want_fix && db > trainset.fix.n) nx = DevMem<unsigned char>(db, what);
        if (nf) trainset.fr = std::move(nf);
        if (nd) trainset.den = std::move(nd);
        if (nx) trainset.fix = std::move(nx);
        if (!want_fix) trainset.fix.reset();      // the fixation store exists only for a set that has them
        trainset.d_first.grow((size_t)x_in->N, "trainset_open: no device memory for the clip table");
        trainset.ev.create();
        trainset.frames.assign(frames, frames + n_videos);
        trainset.base = base;
        for (auto& p : trainset.put) p.assign((size_t)total, 0);
        trainset.format = format; trainset.flags = flags;
        for (int c = 0; c < 3; ++c) trainset.mean[c] = mean_rgb[c];
        trainset.is_open = true; trainset.timed = false;
    }
    void trainset_close() {
        sync_streams();
        trainset = TrainSet();
    }
    // the call's bytes in the staging buffer (queued on the main stream)
    const unsigned char* trainset_stage_bytes(const unsigned char* src, size_t bytes) {
        if (bytes > trainset.u8.n) {
            HIPCHECK(hipStreamSynchronize(stream));      // a queued copy may still read the old buffer
            trainset.u8.grow(bytes, "trainset_put: no device memory for the staging buffer");
        }
        HIPCHECK(hipMemcpyAsync(trainset.u8, src, bytes, hipMemcpyHostToDevice, stream));
        return trainset.u8;
    }
    void trainset_put_frames_u8(int v, int first, const unsigned char* bgr, int n, int H0, int W0) {
        trainset.need_open("trainset_put_frames_u8");
        const int64_t at = trainset.range("trainset_put_frames_u8", v, first, n);
        if (H0 < 1 || W0 < 1) throw P3dError("trainset_put_frames_u8: empty frame");
        if (trainset.format == P3D_TRAINSET_FRAMES_U8) {      // the bytes as they are: the gather normalises
            if (H0 != x_in->H || W0 != x_in->W)
                throw P3dError("trainset_put_frames_u8: the set keeps 8-bit frames (P3D_TRAINSET_FRAMES_U8), which takes frames decoded at the grid's " +
                               std::to_string(x_in->H) + " x " + std::to_string(x_in->W) + ", not " + std::to_string(H0) + " x " + std::to_string(W0));
            HIPCHECK(copy_now(trainset.fr + (size_t)at * ts_frame_bytes(), bgr, (size_t)n * ts_frame_bytes(), hipMemcpyHostToDevice, stream));
        } else {
            const unsigned char* src = trainset_stage_bytes(bgr, (size_t)n * H0 * W0 * 3);
            HIPCHECK(p3d_mapf_frames(src, n, H0, W0, (float*)trainset.fr.p + at * ts_hw() * 3, x_in->H, x_in->W, trainset.mean, stream));
            HIPCHECK(hipStreamSynchronize(stream));
        }
        trainset.mark(0, at, n);
    }
    void trainset_put_frames(int v, int first, const float* x, int n) {
        trainset.need_open("trainset_put_frames");
        const int64_t at = trainset.range("trainset_put_frames", v, first, n);
        if (trainset.format != P3D_TRAINSET_FRAMES_F32)
            throw P3dError("trainset_put_frames: the set keeps 8-bit frames (P3D_TRAINSET_FRAMES_U8); normalised floats need P3D_TRAINSET_FRAMES_F32");
        HIPCHECK(copy_now((float*)trainset.fr.p + at * ts_hw() * 3, x, (size_t)n * ts_frame_bytes(), hipMemcpyHostToDevice, stream));
        trainset.mark(0, at, n);
    }
    void trainset_put_density_u8(int v, int first, const unsigned char* grey, int n, int H0, int W0) {
        trainset.need_open("trainset_put_density_u8");
        const int64_t at = trainset.range("trainset_put_density_u8", v, first, n);
        if (H0 < 1 || W0 < 1) throw P3dError("trainset_put_density_u8: empty map");
        const unsigned char* src = trainset_stage_bytes(grey, (size_t)n * H0 * W0);
        HIPCHECK(p3d_mapf_density_u8(src, n, H0, W0, trainset.den + at * ts_hw(), x_in->H, x_in->W, stream));
        HIPCHECK(hipStreamSynchronize(stream));
        trainset.mark(1, at, n);
    }
    void trainset_put_fixations(int v, int first, const unsigned char* fix, int n) {
        trainset.need_open("trainset_put_fixations");
        const int64_t at = trainset.range("trainset_put_fixations", v, first, n);
        if (!trainset.has_fix()) throw P3dError("trainset_put_fixations: the set was opened without P3D_TRAINSET_FIXATIONS");
        HIPCHECK(copy_now(trainset.fix + at * ts_hw(), fix, (size_t)n * (size_t)ts_hw(), hipMemcpyHostToDevice, stream));
        trainset.mark(2, at, n);
    }
    // validates (nothing launched on a refusal), then queues the table and the one launch between the stage's events.
    // targets: x alone (p3d_trainset_forward), or x, y and -- when the set has them -- the fixations.
    void trainset_gather(const char* who, const int* video, const int* start, int n, bool targets) {
        trainset.need_open(who);
        const int B = x_in->N, T = x_in->D;
        const bool with_fix = targets && trainset.has_fix();
        const unsigned char* const put[3] = {trainset.put[0].data(), targets ? trainset.put[1].data() : nullptr, with_fix ? trainset.put[2].data() : nullptr};
        std::vector<int> first = TrainSet::plan(who, trainset.frames, trainset.base, T, B, video, start, n, put);
        if (with_fix && !d_fix) d_fix = dalloc<unsigned char>(pred->rows());      // address stable from here on: captured steps name it
        trainset.first.swap(first);
        TrainsetGatherArgs a;
        a.format = trainset.format == P3D_TRAINSET_FRAMES_F32 ? TRAINSET_F32 : TRAINSET_U8;
        a.frames = trainset.fr; a.density = trainset.den; a.fixations = trainset.fix;
        a.x = x_in->p; a.y = targets ? d_y : nullptr; a.fix = with_fix ? d_fix : nullptr;
        a.first = trainset.d_first; a.first_host = trainset.first.data(); a.video_host = video; a.start_host = start;
        a.frames_host = trainset.frames.data(); a.n_videos = (int)trainset.frames.size();
        a.B = B; a.T = T; a.hw = ts_hw();
        for (int c = 0; c < 3; ++c) a.mean[c] = trainset.mean[c];
        HIPCHECK(hipMemcpyAsync(trainset.d_first, trainset.first.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, stream));
        trainset.ev.mark(0, stream);
        HIPCHECK(p3d_trainset_gather(a, stream));
        trainset.ev.mark(1, stream);
        if (with_fix) fix_fresh = true;      // the gather is the upload p3d_upload_fixations would have been
        trainset.timed = true;
    }
    // p3d_trainset_step's refusals that do not depend on the clips, ahead of anything that changes state
    void trainset_step_check() const {
        trainset.need_open("trainset_step");
        refuse_swapped("train step");
        if (saliency_needs_fixations() && !trainset.has_fix())
            throw P3dError("trainset_step: the loss has an NSS term (w_nss > 0) and the training set was opened without P3D_TRAINSET_FIXATIONS");
    }
