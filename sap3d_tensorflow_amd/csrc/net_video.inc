// part of net.hip (members of p3d_handle): resident video inference (p3d_video_*; video.hip) with its kept source, its shot table
// (shots.hip) and the temporal stage of its read-out (temporal.hip).  Nothing exists before the first p3d_video_open and nothing
// here runs while no video is open; no step, launch list or captured graph names the stores.  The gather writes the staged x_in,
// whose address never moves, as an upload does.  The host keeps the authoritative counts and which frames were put; the device's
// copy of the counts follows the scatter launches.  Every entry point ends synchronised, so the next call may overwrite the host
// tables.
    // p3d_video_close assigns a fresh one; a p3d_video_open on an open video keeps the stores that are large enough
    struct Video {
        bool is_open = false;
        int F = 0, mode = VIDEO_NEWEST, last = -1;
        DevMem<float> frames, maps; DevMem<int32_t> count_dev;      // the stores: room for at least F frames
        DevMem<unsigned char> u8;                                   // staging of p3d_video_put_frames_u8's bytes; only grows
        // p3d_video_keep_source: the decoded frames [F][H0][W0][3] as they were put, for p3d_video_render.  Off: nothing of it exists
        bool keep = false, u8_put = false;                          // u8_put: a p3d_video_put_frames_u8 has run since the open
        DevMem<unsigned char> source;
        int H0 = 0, W0 = 0;
        std::vector<unsigned char> has_src;                         // [F]: the frame's bytes are in the store
        DevMem<P3dVideoDst> d_dst; DevMem<int> d_src, d_starts;     // the per-call tables, [B*T], [B*T], [B]
        DevMem<int> d_slots;                                        // p3d_video_predict_shots's per-call table [B*T], from its first call
        std::vector<int32_t> count; std::vector<unsigned char> put;
        EventSet<4> ev;                                             // around the last call's gather and scatter (p3d_video_last_ms)
        bool timed = false;
        // the shot table (p3d_video_set_shots, p3d_video_detect_shots): none until installed.  While one is installed the temporal stage
        // filters inside the shots (the *_shots launches of temporal.hip, from a run table that follows the filtered maps in the
        // scratch) and p3d_video_reframe smooths its track inside them; nothing else reads it.
        std::vector<int32_t> shots;                                 // the starts, ascending from 0; empty: no table
        std::vector<int32_t> shot_kinds;                            // P3D_SHOT_* of every shot where p3d_video_detect_transitions installed the table; else empty
        std::vector<int> runs;                                      // the host's copy of the last run table (it outlives the asynchronous upload)

        // What one p3d_video_predict does to the stores, from host state alone (no HIP call): validates as the header says -- the
        // message names the first offending window or frame -- and builds the padded starts, the scatter table and the counts after
        // the call.  put (or null: every frame counts as put) has F entries.
        //
        // shots (or null: p3d_video_predict's plan, windows of T consecutive frames wherever they lie) is the installed table of
        // n_shots starts: the plan of p3d_video_predict_shots ("Shot-aware windows").  Window k then reads slots [k * T + t] = g(k, t),
        // reflected inside its shot, and only its first live [k] slots -- the frames starts[k] + t themselves -- reach the scatter table.
        struct Plan {
            std::vector<int> starts; std::vector<P3dVideoDst> dst; std::vector<int> src; std::vector<int32_t> count;
            std::vector<int> slots, live;      // [B * T], [B]: under a shot table only; the padding clips repeat the last window's slots, live 0
        };
        static int refl(int j, int L) {      // the TEMPORAL paragraph's periodic reflect-101 of j >= 0 into 0 .. L - 1
            if (L == 1) return 0;
            const int m = j % (2 * L - 2);
            return m < L ? m : 2 * L - 2 - m;
        }
        static Plan plan(int mode, int F, int T, int B, int last_start, const int32_t* count, const unsigned char* put,
                         const int* starts, int n_windows, const int32_t* shots = nullptr, int n_shots = 0) {
            if (mode != VIDEO_NEWEST && mode != VIDEO_MEAN) throw P3dError("video: mode " + std::to_string(mode) + " is neither P3D_VIDEO_NEWEST (0) nor P3D_VIDEO_MEAN (1)");
            if (T < 1 || B < 1 || F < T) throw P3dError("video: needs at least T = " + std::to_string(T) + " frames, has " + std::to_string(F));
            if (!starts || !count) throw P3dError("null argument");
            if (shots) {
                if (n_shots < 1 || shots[0] != 0 || shots[n_shots - 1] >= F) throw P3dError("video: the shot table starts at 0 and every shot starts before frame F = " + std::to_string(F));
                for (int i = 1; i < n_shots; ++i)
                    if (shots[i] <= shots[i - 1]) throw P3dError("video: the shot table does not ascend at shot " + std::to_string(i));
            }
            if (n_windows < 1 || n_windows > B) throw P3dError("video: n_windows = " + std::to_string(n_windows) + " is outside 1 .. batch = " + std::to_string(B));
            Plan p;
            if (shots) { p.slots.assign((size_t)B * T, 0); p.live.assign((size_t)B, 0); }
            for (int k = 0; k < n_windows; ++k) {
                const int prev = k ? starts[k - 1] : last_start;
                const std::string w = "video: window " + std::to_string(k) + " starts at " + std::to_string(starts[k]);
                if (!shots && (starts[k] < 0 || starts[k] > F - T)) throw P3dError(w + ", outside [0, F - T = " + std::to_string(F - T) + "]");
                if (shots && (starts[k] < 0 || starts[k] > F - 1)) throw P3dError(w + ", outside [0, F - 1 = " + std::to_string(F - 1) + "]");
                if (starts[k] <= prev)
                    throw P3dError(w + (k ? ", not after window " + std::to_string(k - 1) + "'s " : ", not after the last start accepted, ") + std::to_string(prev));
                if (!shots) {
                    for (int t = 0; put && t < T; ++t)
                        if (!put[starts[k] + t]) throw P3dError(w + " and holds frame " + std::to_string(starts[k] + t) + ", which was never put");
                    continue;
                }
                const int i = (int)(std::upper_bound(shots, shots + n_shots, (int32_t)starts[k]) - shots) - 1;
                const int lo = shots[i], hi = (i + 1 < n_shots ? shots[i + 1] : F) - 1, L = hi - lo + 1;
                if (starts[k] != lo && starts[k] + T - 1 > hi)
                    throw P3dError(w + ", which is neither the first frame of its shot [" + std::to_string(lo) + ", " + std::to_string(hi) + "] nor T - 1 = " +
                                   std::to_string(T - 1) + " frames from its end");
                p.live[(size_t)k] = std::min(T, hi - starts[k] + 1);
                for (int t = 0; t < T; ++t) {
                    const int g = lo + refl(starts[k] - lo + t, L);
                    if (put && !put[g]) throw P3dError(w + " and reads frame " + std::to_string(g) + ", which was never put");
                    p.slots[(size_t)k * T + t] = g;
                }
            }
            for (int k = n_windows; shots && k < B; ++k)      // the padding clips repeat the last window's slot row and fold nothing
                std::copy(p.slots.begin() + (size_t)(n_windows - 1) * T, p.slots.begin() + (size_t)n_windows * T, p.slots.begin() + (size_t)k * T);
            const auto live = [&](int k) { return shots ? p.live[(size_t)k] : T; };
            p.starts.assign(starts, starts + n_windows);
            p.starts.resize((size_t)B, starts[n_windows - 1]);      // the padding clips repeat the last window
            p.count.assign(count, count + F);
            const int f0 = starts[0];
            int span = 0;      // starts ascend and a window ends no earlier than the one before it: the last window's end
            for (int k = 0; k < n_windows; ++k) span = std::max(span, starts[k] + live(k) - f0);
            std::vector<int> n((size_t)span, 0), row((size_t)span, -1);
            for (int k = 0; k < n_windows; ++k)
                for (int t = 0; t < live(k); ++t) ++n[(size_t)(starts[k] + t - f0)];
            int nsrc = 0;
            for (int i = 0; i < span; ++i) {      // rows ascending by frame; NEWEST: only frames nothing has written, their first contributor
                const int before = count[f0 + i];
                if (n[(size_t)i] == 0 || (mode == VIDEO_NEWEST && before != 0)) continue;
                const int take = mode == VIDEO_MEAN ? n[(size_t)i] : 1;
                row[(size_t)i] = (int)p.dst.size();
                p.dst.push_back({f0 + i, before, nsrc, 0});
                nsrc += take;
                p.count[(size_t)(f0 + i)] = mode == VIDEO_MEAN ? before + take : 1;
            }
            p.src.assign((size_t)nsrc, 0);
            for (int k = 0; k < n_windows; ++k)      // ascending k within every frame
                for (int t = 0; t < live(k); ++t) {
                    const int r = row[(size_t)(starts[k] + t - f0)];
                    if (r < 0) continue;
                    P3dVideoDst& d = p.dst[(size_t)r];
                    if (mode == VIDEO_NEWEST && d.n == 1) continue;
                    p.src[(size_t)(d.first + d.n++)] = k * T + t;
                }
            return p;
        }

        void need_open(const char* who) const {
            if (!is_open) throw P3dError(std::string(who) + ": no video is open (p3d_video_open)");
        }
        void range(const char* who, int first, int n) const {
            if (n < 1 || first < 0 || first > F - n)
                throw P3dError(std::string(who) + ": frames " + std::to_string(first) + " .. " + std::to_string((int64_t)first + n - 1) +
                               " are outside [0, " + std::to_string(F) + ")");
        }
        // Refuses a frame with count 0.
        void need_predicted(const char* who, int first, int n) const {
            for (int f = first; f < first + n; ++f)
                if (count[(size_t)f] == 0) throw P3dError(std::string(who) + ": frame " + std::to_string(f) + " has no prediction yet (count 0)");
        }
        // the source store goes with the video it belongs to
        void source_drop() {
            source.reset();
            H0 = W0 = 0; keep = false; u8_put = false;
            has_src.clear();
        }
        void keep_source(int on) {
            need_open("video_keep_source");
            if (u8_put) throw P3dError("video_keep_source: frames were already put with p3d_video_put_frames_u8; set it right after p3d_video_open");
            keep = on != 0;
        }
    } video;
    // around the signal and the decision of the last p3d_video_detect_shots.  They outlive the video: p3d_video_shots_last_ms asks
    // for no open one
    struct ShotsTimer { EventSet<3> ev; bool timed = false; } shots_timer;
    int64_t vid_frame_elems() const { return (int64_t)x_in->H * x_in->W * 3; }
    int64_t vid_hw() const { return (int64_t)pred->H * pred->W; }

    void video_open(int frames, int mode) {
        const int T = x_in->D, B = x_in->N;
        if (mode != VIDEO_NEWEST && mode != VIDEO_MEAN) throw P3dError("video_open: mode " + std::to_string(mode) + " is neither P3D_VIDEO_NEWEST (0) nor P3D_VIDEO_MEAN (1)");
        if (frames < T) throw P3dError("video_open: " + std::to_string(frames) + " frames, a window needs " + std::to_string(T));
        if ((int64_t)frames > INT64_MAX / 4 / vid_frame_elems()) throw P3dError("video_open: the frame store is not addressable");
        sync_streams();
        if ((size_t)frames > video.count_dev.n) {      // the new stores first: a failed allocation changes nothing
            const std::string what = "video_open: no device memory for " + std::to_string(frames) + " frames";
            DevMem<float> nf((size_t)frames * vid_frame_elems(), what), nm((size_t)frames * vid_hw(), what);
            DevMem<int32_t> nc((size_t)frames, what);
            video.frames = std::move(nf); video.maps = std::move(nm); video.count_dev = std::move(nc);
        }
        video.d_dst.grow((size_t)B * T, "video_open: no device memory for the scatter table");
        video.d_src.grow((size_t)B * T, "video_open: no device memory for the scatter table");
        video.d_starts.grow((size_t)B, "video_open: no device memory for the window table");
        video.ev.create();
        HIPCHECK(fill_now(video.count_dev, 0, (size_t)frames * 4, stream));
        video.count.assign((size_t)frames, 0);
        video.put.assign((size_t)frames, 0);
        video.source_drop();
        video.shots.clear();
        video.shot_kinds.clear();
        video.F = frames; video.mode = mode; video.last = -1; video.is_open = true; video.timed = false;
    }
    void video_close() {
        sync_streams();
        video = Video();
    }
    void video_put_frames(int first, const float* x, int n) {
        video.need_open("video_put_frames");
        video.range("video_put_frames", first, n);
        HIPCHECK(copy_now(video.frames + (int64_t)first * vid_frame_elems(), x, (size_t)n * vid_frame_elems() * 4, hipMemcpyHostToDevice, stream));
        std::fill(video.put.begin() + first, video.put.begin() + first + n, (unsigned char)1);
        if (!video.has_src.empty()) std::fill(video.has_src.begin() + first, video.has_src.begin() + first + n, (unsigned char)0);      // floats have no source
    }
    void video_put_frames_u8(int first, const unsigned char* bgr, int n, int H0, int W0, const float mean_rgb[3]) {
        video.need_open("video_put_frames_u8");
        video.range("video_put_frames_u8", first, n);
        if (H0 < 1 || W0 < 1) throw P3dError("video_put_frames_u8: empty frame");
        const size_t bytes = (size_t)n * H0 * W0 * 3;
        if (video.keep) {      // the upload lands in the source store and the normalising launch reads it there
            const size_t frame = (size_t)H0 * W0 * 3;
            if (!video.source) {
                video.source = DevMem<unsigned char>((size_t)video.F * frame, "video_put_frames_u8: no device memory for the source store of " + std::to_string(video.F) +
                                                     " frames of " + std::to_string(H0) + " x " + std::to_string(W0));
                video.H0 = H0; video.W0 = W0;
                video.has_src.assign((size_t)video.F, 0);
            } else if (H0 != video.H0 || W0 != video.W0) {
                throw P3dError("video_put_frames_u8: the source store holds " + std::to_string(video.H0) + " x " + std::to_string(video.W0) + " frames, the call puts " +
                               std::to_string(H0) + " x " + std::to_string(W0));
            }
            unsigned char* at = video.source + (size_t)first * frame;
            HIPCHECK(hipMemcpyAsync(at, bgr, bytes, hipMemcpyHostToDevice, stream));
            HIPCHECK(p3d_mapf_frames(at, n, H0, W0, video.frames + (int64_t)first * vid_frame_elems(), x_in->H, x_in->W, mean_rgb, stream));
            HIPCHECK(hipStreamSynchronize(stream));
            std::fill(video.has_src.begin() + first, video.has_src.begin() + first + n, (unsigned char)1);
        } else {
            if (bytes > video.u8.n) {
                HIPCHECK(hipStreamSynchronize(stream));      // a queued copy may still read the old buffer
                video.u8.grow(bytes, "video_put_frames_u8: no device memory for the staging buffer");
            }
            HIPCHECK(hipMemcpyAsync(video.u8, bgr, bytes, hipMemcpyHostToDevice, stream));
            HIPCHECK(p3d_mapf_frames(video.u8, n, H0, W0, video.frames + (int64_t)first * vid_frame_elems(), x_in->H, x_in->W, mean_rgb, stream));
            HIPCHECK(hipStreamSynchronize(stream));
        }
        video.u8_put = true;
        std::fill(video.put.begin() + first, video.put.begin() + first + n, (unsigned char)1);
    }
    void video_predict(const int* starts, int n_windows) {
        video.need_open("video_predict");
        const int B = x_in->N, T = x_in->D;
        const Video::Plan p = Video::plan(video.mode, video.F, T, B, video.last, video.count.data(), video.put.data(), starts, n_windows);
        video_issue(p, starts[n_windows - 1]);
    }
    // p3d_video_predict_shots: the same call with every window held inside its shot of the installed table
    void video_predict_shots(const int* starts, int n_windows) {
        video.need_open("video_predict_shots");
        if (video.shots.empty()) throw P3dError("video_predict_shots: the open video has no shot table (p3d_video_set_shots, p3d_video_detect_shots)");
        const int B = x_in->N, T = x_in->D;
        if ((int64_t)B * T > 65535) throw P3dError("video_predict_shots: batch * T = " + std::to_string((int64_t)B * T) + " slots, the gather takes 65535");
        const Video::Plan p = Video::plan(video.mode, video.F, T, B, video.last, video.count.data(), video.put.data(), starts, n_windows, video.shots.data(), (int)video.shots.size());
        video.d_slots.grow((size_t)B * T, "video_predict_shots: no device memory for the slot table");
        video_issue(p, starts[n_windows - 1]);
    }
    // One accepted call: the tables up, gather, p3d_predict_windows's pass, scatter; a plan with slots gathers slot by slot.
    void video_issue(const Video::Plan& p, int last) {
        const int B = x_in->N, T = x_in->D;
        const bool by_slots = !p.slots.empty();
        VideoGatherArgs g;
        g.store = video.frames; g.x = x_in->p; g.starts = video.d_starts; g.starts_host = p.starts.data();
        g.B = B; g.T = T; g.F = video.F; g.frame_elems = vid_frame_elems();
        VideoGatherSlotsArgs gs;
        gs.store = video.frames; gs.x = x_in->p; gs.frames = video.d_slots; gs.frames_host = p.slots.data();
        gs.B = B; gs.T = T; gs.F = video.F; gs.frame_elems = vid_frame_elems();
        VideoScatterArgs sc;
        sc.mode = video.mode; sc.pred = pred->p; sc.ld = pred->ld; sc.maps = B * T; sc.hw = vid_hw();
        sc.store = video.maps; sc.count = video.count_dev; sc.F = video.F;
        sc.dst = video.d_dst; sc.src = video.d_src; sc.dst_host = p.dst.data(); sc.src_host = p.src.data();
        sc.ndst = (int)p.dst.size(); sc.nsrc = (int)p.src.size();
        if (by_slots) HIPCHECK(hipMemcpyAsync(video.d_slots, p.slots.data(), p.slots.size() * sizeof(int), hipMemcpyHostToDevice, stream));
        else HIPCHECK(hipMemcpyAsync(video.d_starts, p.starts.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, stream));
        if (sc.ndst) HIPCHECK(hipMemcpyAsync(video.d_dst, p.dst.data(), p.dst.size() * sizeof(P3dVideoDst), hipMemcpyHostToDevice, stream));
        if (sc.ndst) HIPCHECK(hipMemcpyAsync(video.d_src, p.src.data(), p.src.size() * sizeof(int), hipMemcpyHostToDevice, stream));
        video.ev.mark(0, stream);
        if (by_slots) HIPCHECK(p3d_video_gather_slots(gs, stream));
        else HIPCHECK(p3d_video_gather(g, stream));
        video.ev.mark(1, stream);
        Ctx c; c.training = false; c.drop = 0.f; c.update_moving = false; c.per_sample = true; c.s = stream;      // p3d_predict_windows's pass
        run_forward(c);
        if (pred->materialize && last_forward_fused) pred->materialize(stream);
        video.ev.mark(2, stream);
        if (sc.ndst) HIPCHECK(p3d_video_scatter(sc, stream));
        video.ev.mark(3, stream);
        HIPCHECK(hipStreamSynchronize(stream));
        video.count = p.count;
        video.last = last;
        video.timed = true;
    }
    // frames first .. first + n - 1 as the read-out returns them: the map store itself under NEWEST; under MEAN `scratch`
    // ([n][hw], not the store) after the division launches queued here.
    const float* video_finalize(const char* who, int first, int n, float* scratch, hipStream_t s) {
        video.need_open(who);
        video.range(who, first, n);
        video.need_predicted(who, first, n);
        if (video.mode == VIDEO_NEWEST) return video.maps + (int64_t)first * vid_hw();
        for (int done = 0; done < n; done += 32768) {
            VideoMeanArgs a;
            a.sum = video.maps + (int64_t)(first + done) * vid_hw(); a.count = video.count_dev + first + done;
            a.out = scratch + (int64_t)done * vid_hw(); a.n = std::min(32768, n - done); a.hw = vid_hw();
            HIPCHECK(p3d_video_mean(a, s));
        }
        return scratch;
    }

    // ---- temporal smoothing of the video's maps at read-out (p3d_set_video_temporal; temporal.hip) -------
    // Off by default, and off nothing here runs.  The setting is a kind with its radius and taps, or its alpha; the stage is one
    // launch issued by the two read-outs in place of video_finalize, into scratch from the stream pool.
    struct TemporalCfg {
        p3d_video_temporal set{P3D_TEMPORAL_OFF, 0.f, 0, 0.f};      // as given
        int r = 0; std::vector<float> w;                            // GAUSS: the effective radius and w_r .. w_2r
        bool on() const { return set.kind != P3D_TEMPORAL_OFF; }
        // what a setting asks for (include/p3d_hip.h); throws on a setting the header refuses.  Host only.
        static TemporalCfg parse(const p3d_video_temporal* c) {
            TemporalCfg t;
            if (!c || c->kind == P3D_TEMPORAL_OFF) return t;
            if (c->kind == P3D_TEMPORAL_GAUSS) {
                if (!std::isfinite(c->sigma) || !(c->sigma > 0.f)) throw P3dError("video_temporal: GAUSS needs a finite sigma > 0");
                if (c->radius < 0 || c->radius > P3D_TEMPORAL_MAX_RADIUS)
                    throw P3dError("video_temporal: radius must be in [0, " + std::to_string(P3D_TEMPORAL_MAX_RADIUS) + "]");
                int r = c->radius;
                if (r == 0) {      // RADIUS of the postprocess section
                    const double k = std::rint(8.0 * (double)c->sigma + 1.0);
                    if (k > 2.0 * P3D_TEMPORAL_MAX_RADIUS + 1.0)
                        throw P3dError("video_temporal: sigma asks for a radius above " + std::to_string(P3D_TEMPORAL_MAX_RADIUS) + "; give a radius");
                    r = ((int)k | 1) / 2;
                }
                if (r < 1) throw P3dError("video_temporal: sigma asks for radius 0; give a radius");
                const std::vector<float> taps = PostCfg::taps(c->sigma, r);
                t.r = r;
                t.w.assign(taps.begin() + r, taps.end());
                t.set = p3d_video_temporal{P3D_TEMPORAL_GAUSS, c->sigma, c->radius, 0.f};
            } else if (c->kind == P3D_TEMPORAL_EMA) {
                if (!std::isfinite(c->alpha) || !(c->alpha >= 0.f && c->alpha < 1.f)) throw P3dError("video_temporal: EMA needs alpha in [0, 1)");
                t.set = p3d_video_temporal{P3D_TEMPORAL_EMA, 0.f, 0, c->alpha};
            } else {
                throw P3dError("video_temporal: kind " + std::to_string(c->kind) + " is none of P3D_TEMPORAL_OFF (0), GAUSS (1), EMA (2)");
            }
            return t;
        }
        // the read-out's refusals for frames first .. first + n - 1 of F (count [F], host): r > F - 1, a needed frame of count 0
        static void check(const char* who, const TemporalCfg& t, int F, int first, int n, const int32_t* count) {
            if (n < 1 || first < 0 || first > F - n)
                throw P3dError(std::string(who) + ": frames " + std::to_string(first) + " .. " + std::to_string((int64_t)first + n - 1) +
                               " are outside [0, " + std::to_string(F) + ")");
            int lo = 0, hi = first + n - 1;
            if (t.set.kind == P3D_TEMPORAL_GAUSS) {
                if (t.r > F - 1)
                    throw P3dError(std::string(who) + ": the temporal radius " + std::to_string(t.r) + " exceeds F - 1 = " + std::to_string(F - 1));
                lo = std::max(0, first - t.r);
                hi = std::min(F - 1, first + n - 1 + t.r);
            }
            for (int f = lo; f <= hi; ++f)
                if (count[f] < 1)
                    throw P3dError(std::string(who) + ": the temporal filter needs frame " + std::to_string(f) + ", which has no prediction yet (count 0)");
        }
        static VideoTemporalArgs args(const TemporalCfg& t, const float* store, const int32_t* count_dev, float* out, int F, int64_t hw,
                                               int first, int n) {
            VideoTemporalArgs a;
            a.kind = t.set.kind; a.store = store; a.count = count_dev; a.out = out; a.F = F; a.hw = hw; a.first = first; a.n = n;
            a.r = t.r; a.alpha = t.set.alpha;
            for (size_t d = 0; d < t.w.size() && d <= (size_t)TEMPORAL_MAX_RADIUS; ++d) a.w[d] = t.w[d];
            return a;
        }
        // the same refusals under a shot table: the reflections stay inside a shot, so r > F - 1 is no refusal, and only frames of the
        // shots that are read are needed
        static void check_shots(const char* who, const TemporalCfg& t, int F, int first, int n, const int32_t* count,
                                         const int32_t* starts, int n_shots) {
            if (n < 1 || first < 0 || first > F - n)
                throw P3dError(std::string(who) + ": frames " + std::to_string(first) + " .. " + std::to_string((int64_t)first + n - 1) +
                               " are outside [0, " + std::to_string(F) + ")");
            const int last = first + n - 1;
            for (int k = 0; k < n_shots; ++k) {
                const int lo = starts[k], hi = (k + 1 < n_shots ? starts[k + 1] : F) - 1;
                if (hi < first || lo > last) continue;
                const int a = std::max(first, lo), b = std::min(last, hi);
                const int from = t.set.kind == P3D_TEMPORAL_GAUSS ? std::max(lo, a - t.r) : lo, to = t.set.kind == P3D_TEMPORAL_GAUSS ? std::min(hi, b + t.r) : b;
                for (int f = from; f <= to; ++f)
                    if (count[f] < 1)
                        throw P3dError(std::string(who) + ": the temporal filter needs frame " + std::to_string(f) + ", which has no prediction yet (count 0)");
            }
        }
    };
    struct Temporal { TemporalCfg cfg; EventSet<2> ev; bool timed = false; } temporal;      // the events exist from the first run on
    void set_video_temporal(const p3d_video_temporal* c) { temporal.cfg = TemporalCfg::parse(c); }      // (refuses before anything changes)
    void video_temporal_check(const char* who, int first, int n) const {
        video.need_open(who);
        if (!video.shots.empty()) TemporalCfg::check_shots(who, temporal.cfg, video.F, first, n, video.count.data(), video.shots.data(), (int)video.shots.size());
        else TemporalCfg::check(who, temporal.cfg, video.F, first, n, video.count.data());
    }
    // floats of scratch behind the n filtered maps that the run table of a read of n frames may take: at most a run a frame and one
    // more a shot, four ints each
    size_t video_temporal_table(int n) const { return video.shots.empty() ? 0 : (size_t)n * 8; }
    // the filtered frames first .. first + n - 1 in `scratch` [n][hw]: one launch between the stage's events
    const float* video_temporal(const char* who, int first, int n, float* scratch, hipStream_t s) {
        video_temporal_check(who, first, n);
        temporal.ev.create();
        const VideoTemporalArgs a = TemporalCfg::args(temporal.cfg, video.maps, video.mode == VIDEO_MEAN ? video.count_dev : nullptr, scratch, video.F,
                                                  vid_hw(), first, n);
        if (!video.shots.empty()) {
            video.runs = p3d_video_temporal_runs(a.kind, a.r, a.hw, video.F, first, n, video.shots.data(), (int)video.shots.size());
            if (video.runs.size() > video_temporal_table(n)) throw P3dError(std::string(who) + ": the run table outgrew its scratch");
            int* table = reinterpret_cast<int*>(scratch + (size_t)n * (size_t)vid_hw());
            HIPCHECK(hipMemcpyAsync(table, video.runs.data(), video.runs.size() * sizeof(int), hipMemcpyHostToDevice, s));
            temporal.ev.mark(0, s);
            HIPCHECK(p3d_video_temporal_shots_launch(a, table, (int)(video.runs.size() / 4), s));
            temporal.ev.mark(1, s);
            temporal.timed = true;
            return scratch;
        }
        temporal.ev.mark(0, s);
        HIPCHECK(p3d_video_temporal_launch(a, s));
        temporal.ev.mark(1, s);
        temporal.timed = true;
        return scratch;
    }
