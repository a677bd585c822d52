// part of net.hip (members of p3d_handle): execution -- forward, loss, the backward scheduler (side-stream filter gradients, parking,
// bucket hand-over to the all-reduce, the two-part optimiser step), step graphs, uploads / downloads.  tests/test_gpu_schedule.py
// checks the stream operations this file issues as a happens-before graph.
    // ---- execution -------------------------------------------------------------------------------
    // P3D_DEBUG_SYNC=1: synchronise and log after every op (fault isolation, not for timing)
    void debug_sync(const char* dir, const Op& op, const Ctx& c) {
        if (!runtime_env().debug_sync) return;
        fprintf(stderr, "[p3d] %s %s (%s) ...", dir, op.name.c_str(), op.kind.c_str());
        fflush(stderr);
        HIPCHECK(hipStreamSynchronize(c.s));
        fprintf(stderr, " ok\n");
        fflush(stderr);
    }
    void run_forward(const Ctx& c) {
        sib_pending.clear();          // (a pass that threw between the two siblings of an ST_B pair must not hand its launch to this one)
        if (stats_count) HIPCHECK(fill_async(stats_arena, 0, (size_t)stats_count * sizeof(double), c.s, "statistics"));
        if (zf_bytes) HIPCHECK(fill_async(zf, 0, zf_bytes, c.s, "forward-arena"));
        Ctx cz = c; cz.z0 = zf; cz.z1 = zf + zf_bytes;
        cz.fuse = fuse_bn && !c.per_sample && !c.dry;
        last_forward_fused = cz.fuse;
        if (!c.dry) pred_ready = true;
        const bool no_side_f = runtime_env().no_side_stream;
        cz.side = (c.prof || no_side_f || c.dry) ? nullptr : side_stream;      // ST_B sibling convs overlap
        const Ctx& c2 = cz;
        for (auto& op : ops) {
            if (c.prof) c.prof->cur_op = op.name;
            op.fwd(c2);
            debug_sync("fwd", op, c);
        }
    }
    // p3d_set_loss's kinds 0-2 into d_loss / d_dlogits.  Each rank's loss is a sum over its own clips, so under data parallelism
    // the summed gradients are still the global batch's.
    LossArgs loss_args() const {
        return {loss_kind, logits->p, pred->p, d_y, (long)pred->rows(), head_sigmoid ? 1 : 0, d_loss, d_dlogits};
    }
    void run_loss(const Ctx& c) {
        HIPCHECK(fill_async(d_loss, 0, sizeof(double), c.s, "loss"));
        if (!c.dry) last_loss_kind = loss_kind;
        if (loss_kind == P3D_LOSS_KLD_CC) return run_map_loss(c);
        if (loss_kind == P3D_LOSS_SALIENCY) return run_saliency_loss(c);
        const LossArgs a = loss_args();
        const LaunchDesc d = p3d_loss_desc(a);
        launch(c, d.kernel, d.flops, d.bytes, [&]() { return p3d_loss(a, c.s); });
    }
    // P3D_LOSS_KLD_CC (map_loss.hip): w_kld KL + w_cc (1 - CC) per [H, W] map, summed over the B*T maps of this rank, so the
    // summed gradients under data parallelism are still the global batch's.  Three launches over the same grid; each reads s
    // (pred, or the raw output through a sigmoid: +3 operations) and the target.  Per element: sums 2 operations; terms ~18
    // (two double divisions, a log, the centred products); dlogits ~20, and a store.
    void run_map_loss(const Ctx& c) {
        const double rows = (double)pred->rows();
        const int ts = head_sigmoid ? 1 : 0;
        const double sg = ts ? 0.0 : 3.0;
        const MapLossArgs a = p3d_map_loss_args(logits->p, pred->p, d_y, (long long)pred->N * pred->D, (long long)pred->H * pred->W, ts,
                                                kld_weight, cc_weight, d_loss, d_dlogits, d_map_scratch, d_map_cnt);
        launch(c, "map_loss_sums_kernel", rows * (2.0 + sg), rows * 8.0, [&]() { return p3d_map_loss_launch(0, a, c.s); });
        launch(c, "map_loss_terms_kernel", rows * (18.0 + sg), rows * 8.0, [&]() { return p3d_map_loss_launch(1, a, c.s); });
        launch(c, "map_loss_grad_kernel", rows * (20.0 + sg), rows * 12.0, [&]() { return p3d_map_loss_launch(2, a, c.s); });
    }
    // P3D_LOSS_SALIENCY (map_loss.hip): the same with w_nss (-NSS) + w_sim (1 - SIM) per map and the fixation bytes of
    // p3d_upload_fixations as a third input, read (a byte per element, in the first and last launch) only when w_nss > 0.  Per
    // element on top of the above: sums ~6 (two minima, two maxima, the fixated count and sum); terms ~6 (two double divisions,
    // a compare); dlogits ~12.
    bool saliency_needs_fixations() const { return loss_kind == P3D_LOSS_SALIENCY && sal_nss > 0.f; }
    // fresh: the entry point brings new x / y from the host, so the fixations must be new too (a stale map must not train silently)
    void check_fixations(bool fresh) const {
        if (!saliency_needs_fixations()) return;
        if (!d_fix) throw P3dError("the loss has an NSS term (w_nss > 0) and no fixation maps were uploaded: p3d_upload_fixations");
        if (fresh && !fix_fresh)
            throw P3dError("the loss has an NSS term (w_nss > 0) and the fixation maps are those of an earlier batch: "
                           "p3d_upload_fixations before every p3d_train_step / p3d_backward");
    }
    SaliencyLossArgs saliency_loss_args() const {
        return p3d_saliency_loss_args(logits->p, pred->p, d_y, d_fix, (long long)pred->N * pred->D, (long long)pred->H * pred->W,
                                      head_sigmoid ? 1 : 0, sal_kld, sal_cc, sal_nss, sal_sim, d_loss, d_dlogits, d_sal_scratch, d_sal_cnt);
    }
    void run_saliency_loss(const Ctx& c) {
        check_fixations(false);
        if (!d_sal_scratch) throw P3dError("saliency loss: scratch was not planned (p3d_set_loss)");
        const double rows = (double)pred->rows();
        const double sg = head_sigmoid ? 0.0 : 3.0, fb = sal_nss > 0.f ? 1.0 : 0.0;
        const SaliencyLossArgs a = saliency_loss_args();
        launch(c, "saliency_loss_sums_kernel", rows * (8.0 + sg), rows * (8.0 + fb), [&]() { return p3d_saliency_loss_launch(0, a, c.s); });
        launch(c, "saliency_loss_terms_kernel", rows * (24.0 + sg), rows * 8.0, [&]() { return p3d_saliency_loss_launch(1, a, c.s); });
        launch(c, "saliency_loss_grad_kernel", rows * (32.0 + sg), rows * (12.0 + fb), [&]() { return p3d_saliency_loss_launch(2, a, c.s); });
    }
    // with_adam: the optimiser step is part of the call and split in two -- every variable but the first op's (and those its
    // backward reads, adam_split) is updated while that op's filter gradient (the stem's: the last launch of the pass, alone on
    // the side stream) is still running, the rest after it.  Returns whether Adam ran (false: the caller launches run_adam).
    // Gradient buffer (248 MB), gradient arena of the activations and the double-precision reduction arena start a backward pass
    // at zero.  A train step knows that a backward pass follows its forward pass: it zeroes them on the side stream while the
    // forward runs (the previous step's optimiser has read the gradients: the side stream is joined before it) instead of
    // ~0.1 ms of fills at the head of the backward on the main stream.
    bool zeroed_early = false;
    hipEvent_t ev_zeroed = nullptr, ev_zero_fork = nullptr;
    void zero_backward_arenas(hipStream_t st, bool with_zb) {
        // (zb holds whatever buffers the backward ops zero-fill before adding into them; it is planned from a dry run and may
        //  name a buffer the forward pass also touches, so it is never zeroed early)
        if (with_zb && zb_bytes) HIPCHECK(fill_async(zb, 0, zb_bytes, st, "backward-arena"));
        HIPCHECK(fill_async(flat_g, 0, (size_t)n_train * sizeof(float), st, "gradients"));
        if (red_count) HIPCHECK(fill_async(red_arena, 0, (size_t)red_count * sizeof(double), st, "reductions"));
    }
    void zero_early(const Ctx& c) {      // call right before run_forward of a train step (not while capturing, not when profiling)
        if (runtime_env().no_side_stream || !side_stream || c.prof || c.dry) return;
        if (!ev_zeroed) HIPCHECK(hipEventCreateWithFlags(&ev_zeroed, local_event_flags()));
        // after everything the main stream has queued so far (the previous step's optimiser and whoever read the gradients)
        if (!ev_zero_fork) HIPCHECK(hipEventCreateWithFlags(&ev_zero_fork, local_event_flags()));
        HIPCHECK(ev_record(ev_zero_fork, c.s));
        HIPCHECK(ev_wait(side_stream, ev_zero_fork));
        zero_backward_arenas(side_stream, false);
        HIPCHECK(ev_record(ev_zeroed, side_stream));
        zeroed_early = true;
    }
    bool run_backward(const Ctx& c0, bool allreduce, bool with_adam = false) {
        Ctx c = c0; c.z0 = zb; c.z1 = zb + zb_bytes;
        c.fuse = last_forward_fused && !c.dry;       // the backward follows the forward that produced the activations
        c.fuse_bwd = c.fuse && fuse_bn_bwd;
        bool adam_done = false;
        const bool no_side = runtime_env().no_side_stream;
        c.side = (c.prof || no_side) ? nullptr : side_stream;      // per-launch profiling keeps one stream
        if (zeroed_early) {          // the train step zeroed the backward's arenas on the side stream, beside its forward pass
            zeroed_early = false;
            HIPCHECK(ev_wait(c.s, ev_zeroed));
            if (zb_bytes) HIPCHECK(fill_async(zb, 0, zb_bytes, c.s, "backward-arena"));
        } else {
            zero_backward_arenas(c.s, true);
        }
        for (auto& a : acts) if (a.stem_link) a.stem_link->pending = false;      // (a pass that threw must not leave its hand-over to this one)
        int64_t hi = n_train;                        // grads in [hi, n_train) are already handed to the comm stream
        size_t own_pos = own_sorted.size();
        wq.clear(); wq_flushes = 0;
        // The decoder's backward saturates the chip (deconv input gradients at 80+ TFLOP/s) while the encoder's is a chain of
        // small launches that leaves most CUs idle.  The decoder's side-stream jobs (filter and bias gradients) are therefore
        // parked and released when the walk reaches the encoder, where they fill idle CUs instead of halving the rate of the
        // main stream's big kernels.  Grouping and summation order do not change, only the launch time.
        // Parking is bounded by what that phase can absorb (defer_budget, finalize_build): a head that is many times the
        // encoder (unet++, the GN nets) parks its first jobs only, and nothing is parked when the encoder's own launches fill
        // the chip (32x224x224 clips).
        std::vector<std::pair<hipEvent_t, std::function<void(const Ctx&)>>> parked;
        bool early_adam = false, early_comm = false;
        // the applying micro-step of p3d_set_grad_accum: flat_g = acc + g, every element once, after its last producer and before
        // its first reader (all-reduce, sumsq_range, adam_range).  With a communicator reduce_range finishes each bucket on the
        // comm stream ahead of its collective; without one the main stream does, in the optimiser's two ranges (below)
        const bool finish_main = c.acc_finish && !(allreduce && comm && !bucket_hook);
        static const bool no_defer = p3d_tune_env("P3D_DEFER_SIDE") && atoi(p3d_tune_env("P3D_DEFER_SIDE")) == 0;
        const bool defer_on = c.side && !no_defer && defer_release_op > 0 && defer_budget > 0;
        parked_flops = 0;
        auto release_parked = [&]() {
            c.defer = nullptr;
            // ONE fork for all of them: the main stream does not advance between the jobs, so the first job's event orders every later
            // one too (they follow it in side-stream order).  A fork per job is the same order with redundant edges -- and a captured
            // step graph with eight successors on the node before the release replayed with wrong encoder gradients on ROCm 7.2
            // (tests/test_gpu_determinism.py, round 5: right again with a join behind the release or with this single fork)
            bool first = true;
            for (auto& job : parked) {
                if (first || !c.side) on_side_stream(c, job.first, job.second);
                else { Ctx sc = c; sc.s = c.side; job.second(sc); }
                first = false;
            }
            parked.clear();
        };
        for (int i = (int)ops.size() - 1; i >= 0; --i) {
            if (c.prof) c.prof->cur_op = ops[i].name;
            c.bwd_op = ops[i].name.c_str();
            if (i == 1) flush_wgrads(c);      // what is still queued runs beside the stem's normalisation backward, not after it
            if (i == 0 && adam_split > 0 && adam_split < n_train && c.side && !c.dry) {
                // every gradient at offsets >= adam_split is final once the side stream has drained what is queued so far:
                // hand that range over now, so that neither its all-reduce nor its Adam waits for the first op's filter gradient
                flush_wgrads(c);
                if (c.defer || !parked.empty()) release_parked();
                const bool reduce = allreduce && (comm || bucket_hook);
                if (hi > adam_split) {
                    if (reduce) reduce_range(adam_split, hi, c, 1);
                    hi = adam_split;
                }
                static const bool no_split = p3d_tune_env("P3D_SPLIT_ADAM") && atoi(p3d_tune_env("P3D_SPLIT_ADAM")) == 0;     // A/B runs
                if (with_adam && !no_split) {
                    // what the first Adam part has to wait for is marked NOW, before the first op's filter gradient goes to the
                    // side stream; the part itself is enqueued after that op's backward (below), so that the two overlap --
                    // enqueued here, the filter gradient's fork event would sit behind Adam on the main stream and the tail of
                    // the step would be Adam, then the filter gradient, then the second Adam part, one after the other
                    HIPCHECK(ev_record(ev_side_early, c.side));
                    early_comm = reduce && comm && !bucket_hook;
                    if (early_comm) HIPCHECK(ev_record(ev_comm_early, comm_stream));
                    early_adam = true;
                }
            }
            if (defer_on) {
                if (i > defer_release_op) c.defer = parked_flops < defer_budget ? &parked : nullptr;
                else if (c.defer || !parked.empty()) release_parked();
            }
            ops[i].bwd(c);
            debug_sync("bwd", ops[i], c);
            if (early_adam) {
                early_adam = false;
                HIPCHECK(ev_wait(c.s, ev_side_early));
                if (early_comm) HIPCHECK(ev_wait(c.s, ev_comm_early));
                if (finish_main) grad_accum_range(c, GACC_FINISH, adam_split, n_train);      // final since ev_side_early
                if (clip_on()) {
                    // clipping: no update before every gradient is final; the slot takes the norm's first range instead
                    sumsq_range(c, adam_split, n_train);
                } else {
                    adam_begin(c);
                    adam_range(c, adam_split, n_train);
                }
                adam_done = true;
            }
            {
                // gradients at flat offsets >= lo belong to ops i.. only, so they are final now.  The walk (and the flush
                // of queued filter gradients at every bucket boundary) runs with or without a communicator, so that the
                // grouping of filter gradients -- hence every bit of the result -- does not depend on the world size or on
                // whether the call is a train step or the parity hook p3d_backward.
                while (own_pos > 0 && own_sufmin[own_pos - 1] >= i) --own_pos;
                const int64_t lo = own_pos < own_sorted.size() ? own_sorted[own_pos].first : n_train;
                if ((hi > lo && hi - lo >= bucket_floats) || i == 0) {
                    const int64_t start = (i == 0) ? 0 : lo;
                    flush_wgrads(c);                 // the bucket's queued filter gradients must be on the side stream first
                    if (i == 0 && (c.defer || !parked.empty())) release_parked();
                    // while jobs are parked their gradients are not on the side stream yet: the range stays with the walk
                    // and is handed over at the first boundary after the release
                    if (parked.empty()) {
                        if (hi > start && allreduce && (comm || bucket_hook)) reduce_range(start, hi, c, i);
                        hi = start;
                    }
                }
            }
        }
        flush_wgrads(c);
        if (c.defer || !parked.empty()) release_parked();
        // the stem's normalisation backward hands its apply pass to the stem conv's filter gradient through host state: the conv's
        // backward (the op right after it in this walk) must have taken it (ADVICE round 4)
        for (auto& a : acts)
            if (a.stem_link && a.stem_link->pending) {
                a.stem_link->pending = false;
                throw P3dError("the stem BatchNorm's backward left its apply pass to a filter gradient that never ran (" + a.name + ")");
            }
        static const bool tune_tail = p3d_tune_env("P3D_TUNE_TAIL") != nullptr;   // diagnostic: how long the side stream outlasts the main one
        static hipEvent_t tail_main = nullptr, tail_side = nullptr;
        if (tune_tail && c.side && !c.dry) {
            if (!tail_main) { HIPCHECK(hipEventCreate(&tail_main)); HIPCHECK(hipEventCreate(&tail_side)); }
            HIPCHECK(ev_record(tail_main, c.s));
            HIPCHECK(ev_record(tail_side, c.side));
        }
        if (c.side) {       // weight gradients must be complete before the optimiser (and the next step)
            HIPCHECK(ev_record(ev_side_done, c.side));
            HIPCHECK(ev_wait(c.s, ev_side_done));
        }
        if (tune_tail && c.side && !c.dry) {
            HIPCHECK(hipEventSynchronize(tail_main)); HIPCHECK(hipEventSynchronize(tail_side));
            float ms = 0.f;
            const hipError_t e = hipEventElapsedTime(&ms, tail_main, tail_side);
            fprintf(stderr, "[p3d tune] side stream ends %.3f ms after the main stream's backward%s (adam_split %lld)\n", e == hipSuccess ? ms : -1.f,
                    adam_done ? " + first Adam part" : "", (long long)adam_split);
        }
        if (allreduce && (comm || bucket_hook)) {
            if (hi > 0) reduce_range(0, hi, c, 0);
            if (comm && !bucket_hook) {
                HIPCHECK(ev_record(ev_comm_done, comm_stream));
                HIPCHECK(ev_wait(c.s, ev_comm_done));
            }
        }
        if (finish_main) grad_accum_range(c, GACC_FINISH, 0, adam_done ? adam_split : n_train);      // the rest: the side stream is joined
        if (adam_done && clip_on()) {      // the norm's second range folds; then the optimiser's usual two ranges on the scale
            sumsq_range(c, 0, adam_split);
            adam_begin(c);
            adam_range(c, adam_split, n_train);
        }
        if (adam_done) adam_range(c, 0, adam_split);
        return adam_done;
    }
    // audit hook (p3d_debug_bucket_audit): called in place of the collective with the range and the op whose backward
    // had just run when the bucket was handed over
    std::function<void(int64_t, int64_t, int)> bucket_hook;
    void reduce_range(int64_t lo, int64_t hi, const Ctx& c, int after_op) {
        if (bucket_hook) { bucket_hook(lo, hi, after_op); return; }
        HIPCHECK(ev_record(ev_bucket, c.s));
        HIPCHECK(ev_wait(comm_stream, ev_bucket));
        if (c.side) {       // the bucket's weight gradients were queued on the side stream
            HIPCHECK(ev_record(ev_side_bucket, c.side));
            HIPCHECK(ev_wait(comm_stream, ev_side_bucket));
        }
        if (c.acc_finish) {      // p3d_set_grad_accum: each rank's accumulated sum is what the ranks add up
            Ctx cc = c; cc.s = comm_stream; cc.side = nullptr;
            grad_accum_range(cc, GACC_FINISH, lo, hi);
        }
        if (g_trace) g_trace->lines.push_back("C " + g_trace->sname(comm_stream) + " allreduce " + std::to_string(lo) + " " + std::to_string(hi));
        Perturb* const pt = g_perturb;
        if (pt) HIPCHECK(pt->before(comm_stream));
        NCCLCHECK(ncclAllReduce(flat_g + lo, flat_g + lo, (size_t)(hi - lo), ncclFloat, ncclSum, comm, comm_stream));
        if (pt) HIPCHECK(pt->after(comm_stream));
    }
    float cur_lr_t = 0.f;
    int64_t adam_split = 0;              // flat offset below which only the first op's variables live (0: no split)
    hipEvent_t ev_side_early = nullptr, ev_comm_early = nullptr;
    // The optimiser (p3d_set_optimizer) runs as the same two parts under every kind; only the kernel differs.  Its step size
    // for step t: Adam's bias-corrected one, the constant lr for Momentum and SGD.
    float opt_step_size(int64_t t) const { return opt_kind == P3D_OPT_ADAM ? adam_step_size(lr, b1, b2, t) : lr; }
    void adam_begin(const Ctx& c) {      // c.lr_dev set: the step size comes from device memory (graph replay), `step` is the caller's
        cur_lr_t = c.lr_dev ? 0.f : opt_step_size(++step);
    }
    // One optimiser launch over the variables in [lo, hi): the update of the current kind, on g + c w when a regularisation term
    // is on; update = false is the gradient-only launch of p3d_backward.
    void adam_range(const Ctx& c, int64_t lo, int64_t hi, bool update = true) {
        if (hi <= lo) return;
        static const bool skip = p3d_tune_env("P3D_TUNE_SKIP_ADAM") != nullptr;      // timing diagnostic (tuning build; the weights stay put)
        if (skip && update) return;
        double decayed = 0.0;
        const OptArgs a = opt_args(lo, hi, update, cur_lr_t, c.lr_dev, &decayed);
        const LaunchDesc d = p3d_opt_desc(a, decayed);
        launch(c, d.kernel, d.flops, d.bytes, [&]() { return p3d_opt_step(a, c.s); });
        if (update && ema_on) ema_range(c, lo, hi);      // the shadows follow their parameters, range by range
    }
    void run_adam(const Ctx& c) {
        if (clip_on()) sumsq_range(c, 0, n_train);
        adam_begin(c);
        adam_range(c, 0, n_train);
    }

    // ---- exponential moving average of the weights (p3d_set_ema) ---------------------------------------
    // flat_ema shadows flat_p (same offsets; allocated when the option is first switched on).  Every optimiser launch of a train
    // step is followed on its stream by one ema_kernel over the same range, so the early range still overlaps the stem's filter
    // gradient; p3d_backward updates nothing.  om (p3d_hip.h): float(1 - decay) in double, or under warm-up 1.f - min(decay,
    // (1 + t) / (10 + t)) in float32 with t the completed optimiser steps including this one -- a launch argument, or under
    // warm-up in a captured step the device float d_om (p3d_set_step_scalars).  Ranks hold the same weights after the
    // all-reduced update, hence the same shadows: nothing is communicated.
    float* flat_ema = nullptr;
    bool ema_on = false, ema_warmup = false, ema_swapped = false;
    double ema_decay = 0.0;
    float* d_om = nullptr;
    float ema_om(int64_t t) const {
        if (!ema_warmup) return (float)(1.0 - ema_decay);
        const float tf = (float)t;
        const float q = (1.f + tf) / (10.f + tf);
        return 1.f - fminf((float)ema_decay, q);
    }
    void ema_range(const Ctx& c, int64_t lo, int64_t hi) {
        if (hi <= lo) return;
        EmaArgs a;
        a.s = flat_ema + lo; a.p = flat_p + lo; a.n = (long)(hi - lo);
        if (c.om_dev && ema_warmup) a.om_dev = c.om_dev;
        else a.om = ema_om(step);      // (adam_begin has counted this step; a captured step with a constant decay never reads `step`)
        const LaunchDesc d = p3d_ema_desc(a);
        launch(c, d.kernel, d.flops, d.bytes, [&]() { return p3d_ema_step(a, c.s); });
    }
    void sync_streams() {
        HIPCHECK(hipStreamSynchronize(stream));
        HIPCHECK(hipStreamSynchronize(side_stream));
        HIPCHECK(hipStreamSynchronize(comm_stream));
    }
    void ema_seed() {      // TF initialises a shadow from its variable
        HIPCHECK(hipMemcpyAsync(flat_ema, flat_p, (size_t)n_train * sizeof(float), hipMemcpyDeviceToDevice, stream));
        HIPCHECK(hipStreamSynchronize(stream));
    }
    void refuse_swapped(const char* what) const {
        if (ema_swapped)
            throw P3dError(std::string(what) + ": parameters and averaged weights are exchanged (p3d_ema_swap); swap back first");
    }
    void set_ema(double decay, bool warmup) {
        refuse_swapped("p3d_set_ema");
        if (!(decay < 0.0) && !(std::isfinite(decay) && decay < 1.0))
            throw P3dError("moving average: decay must be finite with 0 <= decay < 1 (negative: off)");
        sync_streams();
        if (decay < 0.0) {
            ema_on = false;
        } else {
            if (!flat_ema) flat_ema = dalloc<float>(n_train);
            if (!ema_on) ema_seed();
            ema_on = true; ema_decay = decay; ema_warmup = warmup;
        }
        drop_step_graph();      // the launch list differs, and a constant om is a launch argument
    }
    float* ema_ptr(const char* var, int64_t count) {
        if (!ema_on) throw P3dError("moving average: the option is off (p3d_set_ema)");
        if (!var) throw P3dError("null argument");
        auto it = pindex.find(var);
        if (it == pindex.end()) throw P3dError(std::string("no variable named ") + var);
        const Param* p = it->second;
        if (!p->trainable) throw P3dError(std::string(var) + " is not trainable: it has no moving average");
        if (count != p->count)
            throw P3dError(std::string("size mismatch for ") + var + ": got " + std::to_string(count) + ", variable has " +
                           std::to_string(p->count));
        return flat_ema + p->off;
    }
    void ema_swap() {
        if (!ema_on) throw P3dError("moving average: the option is off (p3d_set_ema)");
        sync_streams();
        HIPCHECK(p3d_ema_swap(flat_p, flat_ema, (long long)n_train, stream));
        HIPCHECK(hipStreamSynchronize(stream));
        ema_swapped = !ema_swapped;
    }

    // ---- gradient accumulation over micro-batches (p3d_set_grad_accum) ---------------------------------
    // acc_k >= 2: every train step is micro-step j = acc_pending of a cycle of acc_k.  j < acc_k - 1 accumulates: forward (moving
    // statistics updated), loss, backward without all-reduce or optimiser, then flat_acc = g (j = 0, GACC_STORE) or
    // flat_acc += g (GACC_ADD) over [0, n_train) on the main stream, which has joined the side stream by then (ev_side_done).
    // The next call's zero_early forks from the main stream's tail, so its fill of flat_g stays behind this read.  j = acc_k - 1
    // applies: run_backward (Ctx::acc_finish) writes flat_g = flat_acc + g range by range, and the all-reduce, the
    // regularisation term, the norm, the optimiser and the moving average run on it as on any gradient.  flat_acc (one float
    // per trainable element) is allocated the first time acc_k >= 2 is set.  p3d_backward and the audit hook never touch it.
    float* flat_acc = nullptr;
    int acc_k = 1, acc_pending = 0;
    bool acc_accumulating() const { return acc_k > 1 && acc_pending < acc_k - 1; }
    void grad_accum_range(const Ctx& c, int mode, int64_t lo, int64_t hi) {
        if (hi <= lo) return;
        GradAccumArgs a;
        a.acc = flat_acc + lo; a.g = flat_g + lo; a.n = (long)(hi - lo); a.mode = mode;
        const LaunchDesc d = p3d_grad_accum_desc(a);
        if (g_trace && !c.dry)
            g_trace->lines.push_back("G " + g_trace->sname(c.s) + (mode == GACC_STORE ? " store " : mode == GACC_ADD ? " add " : " finish ") +
                                     std::to_string(lo) + " " + std::to_string(hi));
        launch(c, d.kernel, d.flops, d.bytes, [&]() { return p3d_grad_accum_step(a, c.s); });
    }
    // the tail of an accumulating micro-step, after its run_backward(c, false, false)
    void grad_accum_take(const Ctx& c) {
        grad_accum_range(c, acc_pending == 0 ? GACC_STORE : GACC_ADD, 0, n_train);
        // no term belongs to this micro-step: the loss read after it is the data loss alone, and p3d_last_regularization gives 0
        if (reg_terms) HIPCHECK(fill_async(d_reg, 0, sizeof(double), c.s, "regularisation"));
        ++acc_pending;
    }
    void set_grad_accum(int k) {
        if (k < 1) throw P3dError("gradient accumulation: k must be 1 (off) or larger, not " + std::to_string(k));
        sync_streams();
        if (k > 1 && !flat_acc) flat_acc = dalloc<float>(n_train);
        acc_k = k;
        acc_pending = 0;          // a partial sum is discarded
        drop_step_graph();        // the captured step is not used while k >= 2
    }

    // ---- clip augmentation of the staged inputs (p3d_set_augment) --------------------------------------
    // Off by default, and off nothing here runs.  On, p3d_train_step brings x and y from the host into the scratch copies aug_x /
    // aug_y instead of the staged buffers, copies the fixation bytes there when the loss reads them, and augment.hip's launches
    // write x_in, d_y and d_fix from the scratch -- on the main stream, ahead of the step and outside its launch list: the step
    // (eager or captured) names the staged buffers, whose addresses never move, and never the scratch.  p3d_augment_inputs does
    // the same from the staged buffers themselves (device to device) for the device-resident path.  The decisions are drawn on
    // the host (aug_draw: SplitMix64 of the step's seed and the clip's global index rank * B + b) and reach the kernels as
    // d_aug_tab.  The main stream runs every transfer and launch in order, and every entry point here ends synchronised, so the
    // next call may overwrite aug_tab.
    bool aug_on = false, aug_have = false;
    p3d_augment aug_cfg{0.f, 0.f, 1.f, 0.f, 0.f};
    float* aug_x = nullptr; float* aug_y = nullptr; unsigned char* aug_fix = nullptr;
    P3dAugClip* d_aug_tab = nullptr;
    std::vector<P3dAugClip> aug_tab;      // the last augmentation's decisions (p3d_last_augment)
    EventSet<2> aug_ev;                   // around the last augmentation's launches (p3d_last_augment_ms)
    static bool aug_cfg_valid(const p3d_augment& c) {
        for (float v : {c.p_flip, c.p_reverse, c.min_scale, c.contrast, c.brightness}) if (!std::isfinite(v)) return false;
        return c.p_flip >= 0.f && c.p_flip <= 1.f && c.p_reverse >= 0.f && c.p_reverse <= 1.f && c.min_scale > 0.f && c.min_scale <= 1.f &&
               c.contrast >= 0.f && c.contrast < 1.f && c.brightness >= 0.f;
    }
    static bool aug_cfg_neutral(const p3d_augment& c) {
        return c.p_flip == 0.f && c.p_reverse == 0.f && c.min_scale == 1.f && c.contrast == 0.f && c.brightness == 0.f;
    }
    // draw j of clip g under `seed` (include/p3d_hip.h): SplitMix64's finaliser on seed ^ A5.. + golden * (1 + 8 g + j), 53 bits
    static double aug_uniform(uint64_t seed, uint64_t g, int j) {
        uint64_t z = seed ^ 0xA5A5A5A5A5A5A5A5ull;
        z += 0x9E3779B97F4A7C15ull * (1ull + 8ull * g + (uint64_t)j);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        return (double)(z >> 11) * 0x1.0p-53;
    }
    static P3dAugClip aug_draw(uint64_t seed, uint64_t g, int H, int W, const p3d_augment& c) {
#pragma clang fp contract(off)
        P3dAugClip k;
        k.flip = aug_uniform(seed, g, 0) < (double)c.p_flip ? 1 : 0;
        k.reverse = aug_uniform(seed, g, 1) < (double)c.p_reverse ? 1 : 0;
        const double s = 1.0 - aug_uniform(seed, g, 2) * (1.0 - (double)c.min_scale);
        k.ch = (int)std::min<double>(std::max<double>(std::floor(s * H + 0.5), 1.0), (double)H);
        k.cw = (int)std::min<double>(std::max<double>(std::floor(s * W + 0.5), 1.0), (double)W);
        k.y0 = std::min((int)std::floor(aug_uniform(seed, g, 3) * (double)(H - k.ch + 1)), H - k.ch);      // (u < 1: the cap never binds)
        k.x0 = std::min((int)std::floor(aug_uniform(seed, g, 4) * (double)(W - k.cw + 1)), W - k.cw);
        k.a = (float)(1.0 + (2.0 * aug_uniform(seed, g, 5) - 1.0) * (double)c.contrast);
        k.b = (float)((2.0 * aug_uniform(seed, g, 6) - 1.0) * (double)c.brightness);
        return k;
    }
    void set_augment(const p3d_augment* c) {
        const p3d_augment neutral{0.f, 0.f, 1.f, 0.f, 0.f};
        const p3d_augment want = c ? *c : neutral;
        if (!aug_cfg_valid(want))
            throw P3dError("augmentation: probabilities in [0, 1], 0 < min_scale <= 1, 0 <= contrast < 1, brightness >= 0, all finite");
        if (aug_cfg_neutral(want)) { aug_on = false; aug_have = false; aug_cfg = neutral; return; }
        if (!aug_x) {      // the first switch-on: private scratch, so no captured step names it
            aug_x = dalloc<float>(x_in->rows() * 3);
            aug_y = dalloc<float>(pred->rows());
            aug_fix = dalloc<unsigned char>(pred->rows());
            d_aug_tab = dalloc<P3dAugClip>(x_in->N);
            aug_ev.create();
        }
        if (!aug_on) aug_have = false;
        aug_on = true; aug_cfg = want;
    }
    // hx / hy: the host's x and y (p3d_train_step), or null: the staged buffers are the source (p3d_augment_inputs)
    void augment_staged(uint64_t seed, const float* hx, const float* hy) {
        if (!aug_on) throw P3dError("augmentation: the option is off (p3d_set_augment)");
        const int B = x_in->N, T = x_in->D, H = x_in->H, W = x_in->W;
        const bool with_fix = saliency_needs_fixations();
        if (with_fix && !d_fix) throw P3dError("the loss has an NSS term (w_nss > 0) and no fixation maps were uploaded: p3d_upload_fixations");
        aug_tab.resize((size_t)B);
        for (int b = 0; b < B; ++b) aug_tab[(size_t)b] = aug_draw(seed, (uint64_t)cfg.rank * (uint64_t)B + (uint64_t)b, H, W, aug_cfg);
        const size_t nx = (size_t)x_in->rows() * 3 * sizeof(float), ny = (size_t)pred->rows() * sizeof(float);
        HIPCHECK(hipMemcpyAsync(d_aug_tab, aug_tab.data(), (size_t)B * sizeof(P3dAugClip), hipMemcpyHostToDevice, stream));
        HIPCHECK(hipMemcpyAsync(aug_x, hx ? hx : x_in->p, nx, hx ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, stream));
        HIPCHECK(hipMemcpyAsync(aug_y, hy ? hy : d_y, ny, hy ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, stream));
        if (with_fix) HIPCHECK(hipMemcpyAsync(aug_fix, d_fix, (size_t)pred->rows(), hipMemcpyDeviceToDevice, stream));
        AugArgs a;
        a.x = aug_x; a.y = aug_y; a.fix = with_fix ? aug_fix : nullptr;
        a.x_out = x_in->p; a.y_out = d_y; a.fix_out = with_fix ? d_fix : nullptr;
        a.tab = d_aug_tab; a.tab_host = aug_tab.data();
        a.B = B; a.T = T; a.H = H; a.W = W;
        aug_ev.mark(0, stream);
        for (int st = 0; st < p3d_augment_stages(a); ++st) HIPCHECK(p3d_augment_launch(st, a, stream));
        aug_ev.mark(1, stream);
        aug_have = true;
    }

    // ---- gradient clipping by the global norm (p3d_set_grad_clip) ----------------------------------
    // clip_norm > 0: the step's sum of squares over every trainable element's g' (g + c w under a regularisation term), its
    // norm and scale = clip_norm / max(norm, clip_norm) land in d_clip_res before any optimiser launch, and every optimiser
    // launch reads the scale (OptArgs::gscale).  +inf measures only.  The chunk table: each trainable's [off, off + count) cut
    // at REG_TILE with the variable's coefficient.  Slot padding is in no chunk, so it is never read: nothing here depends on
    // what the filter-gradient kernels leave there.  The cut depends on the flat layout alone, the coefficients on the
    // regularisation settings (set_regularization rebuilds the table).  Every range sumsq_range is called with starts at a
    // variable's offset; the range that starts at 0 is the last one launched and folds the whole table.
    float clip_norm = 0.f;
    bool clip_have = false;              // a step or a backward has written d_clip_res since the option was set
    std::vector<P3dRegTile> clip_tiles;
    std::vector<int64_t> clip_decayed;   // elements with c != 0 in chunks [0, k)
    std::vector<int64_t> clip_elems;     // elements in chunks [0, k)
    P3dRegTile* d_clip_tiles = nullptr;
    double* d_clip_part = nullptr;
    double* d_clip_res = nullptr;        // sumsq, norm; the float scale at [2]
    unsigned* d_clip_cnt = nullptr;
    bool clip_on() const { return clip_norm > 0.f; }
    const float* clip_scale_dev() const { return reinterpret_cast<const float*>(d_clip_res + 2); }
    void build_clip_table() {
        std::vector<const Param*> tr;
        for (const Param* p : porder) if (p->trainable) tr.push_back(p);
        std::sort(tr.begin(), tr.end(), [](const Param* a, const Param* b) { return a->off < b->off; });
        std::vector<P3dRegTile> tiles;
        for (const Param* p : tr) {
            const float c = (float)(reg_coef64(p, P3D_REG_WEIGHT_DECAY) + reg_coef64(p, P3D_REG_L2));      // set_regularization's
            for (int64_t a = p->off, b = p->off + p->count; a < b; a += REG_TILE)
                tiles.push_back({(long long)a, (int)std::min(REG_TILE, b - a), c});
        }
        if (tiles.empty()) throw P3dError("gradient clipping: no trainable variable");
        HIPCHECK(hipStreamSynchronize(stream));      // the table may be in use by queued work
        if (!d_clip_tiles) {
            d_clip_tiles = dalloc<P3dRegTile>((int64_t)tiles.size());
            d_clip_part = dalloc<double>((int64_t)tiles.size());
            d_clip_res = dalloc<double>(3);
            d_clip_cnt = dalloc<unsigned>(1);
            HIPCHECK(fill_async(d_clip_res, 0, 3 * sizeof(double), stream, "gradient-norm"));
            HIPCHECK(fill_async(d_clip_cnt, 0, sizeof(unsigned), stream, "gradient-norm"));
        }
        HIPCHECK(copy_now(d_clip_tiles, tiles.data(), tiles.size() * sizeof(P3dRegTile), hipMemcpyHostToDevice, stream));
        clip_tiles = std::move(tiles);
        clip_decayed.assign(clip_tiles.size() + 1, 0);
        clip_elems.assign(clip_tiles.size() + 1, 0);
        for (size_t k = 0; k < clip_tiles.size(); ++k) {
            clip_elems[k + 1] = clip_elems[k] + clip_tiles[k].len;
            clip_decayed[k + 1] = clip_decayed[k] + (clip_tiles[k].c != 0.f ? clip_tiles[k].len : 0);
        }
    }
    void set_grad_clip(float cn) {
        if (!(cn >= 0.f)) throw P3dError("gradient clipping: clip_norm must be 0 (off), positive or +inf, not negative or NaN");
        HIPCHECK(hipStreamSynchronize(stream));
        clip_norm = cn;
        clip_have = false;
        if (clip_on()) build_clip_table();
        drop_step_graph();      // the threshold is a launch argument, and the launch list differs
    }
    // the launch over the chunks of [lo, hi), which must start and end between variables
    SumsqArgs sumsq_args(int64_t lo, int64_t hi, double* elems, double* decayed) const {
        auto at = [&](int64_t off) {
            return (int)(std::lower_bound(clip_tiles.begin(), clip_tiles.end(), off,
                                          [](const P3dRegTile& t, int64_t o) { return t.off < o; }) - clip_tiles.begin());
        };
        SumsqArgs a;
        a.k0 = at(lo); a.k1 = at(hi);
        if (a.k1 <= a.k0 || clip_tiles[a.k0].off < lo || clip_tiles[a.k1 - 1].off + clip_tiles[a.k1 - 1].len > hi)
            throw P3dError("gradient clipping: range is not on chunk boundaries");
        *elems = (double)(clip_elems[a.k1] - clip_elems[a.k0]);
        *decayed = (double)(clip_decayed[a.k1] - clip_decayed[a.k0]);
        a.g = flat_g; a.p = flat_p; a.tiles = d_clip_tiles; a.tile_base = 0;
        a.part = d_clip_part; a.nfold = lo == 0 ? (int)clip_tiles.size() : 0;
        a.counter = d_clip_cnt; a.res = d_clip_res; a.clip_norm = clip_norm;
        return a;
    }
    void sumsq_range(const Ctx& c, int64_t lo, int64_t hi) {
        if (hi <= lo) return;
        double elems = 0.0, decayed = 0.0;
        const SumsqArgs a = sumsq_args(lo, hi, &elems, &decayed);
        const LaunchDesc d = p3d_grad_sumsq_desc(a, elems, decayed);
        launch(c, d.kernel, d.flops, d.bytes, [&]() { return p3d_grad_sumsq(a, c.s); });
        if (!c.dry && lo == 0) clip_have = true;
    }
    void read_grad_norm(double* sumsq, double* norm, float* scale) {
        if (!clip_on()) throw P3dError("gradient norm: clipping is off (p3d_set_grad_clip)");
        if (!clip_have) throw P3dError("gradient norm: no train step or backward has run since p3d_set_grad_clip");
        double r[3] = {0, 0, 0};
        HIPCHECK(hipMemcpyAsync(r, d_clip_res, sizeof(r), hipMemcpyDeviceToHost, stream));
        HIPCHECK(hipStreamSynchronize(stream));
        if (sumsq) *sumsq = r[0];
        if (norm) *norm = r[1];
        if (scale) memcpy(scale, &r[2], sizeof(float));
    }

    // ---- regularisation (p3d_set_regularization) ---------------------------------------------------
    // The flat range is cut into tiles of one coefficient each: every trainable's slot is cut at REG_TILE, a decayed variable's
    // slot padding is a tile of its own with c = 0.  Every range adam_range is called with starts at a variable's offset, so at
    // a tile.  Each tile's 0.5 c sum(w^2) lands in d_reg_part[tile]; the range that starts at 0, always the last one launched on
    // the stream, folds all of them in tile order into d_reg: the term does not depend on the optimiser split.
    static constexpr int64_t REG_TILE = 8192;
    int reg_terms = 0;
    double reg_wd = 0.0, reg_l2 = 0.0;
    std::vector<P3dRegTile> reg_tiles;
    std::vector<int64_t> reg_decayed;        // elements with c != 0 in tiles [0, k)
    P3dRegTile* d_reg_tiles = nullptr;
    double* d_reg_part = nullptr;
    double* d_reg = nullptr;
    unsigned* d_reg_cnt = nullptr;
    bool gn_net() const {
        return cfg.structure == P3D_STRUCTURE_GN_P3D || cfg.structure == P3D_STRUCTURE_GN_P3D_CONCAT ||
               cfg.structure == P3D_STRUCTURE_GN_P3D_DECODER;
    }
    int reg_count(int cls) const {
        int k = 0;
        for (const Param* p : porder) k += p->trainable && p->reg == cls;
        return k;
    }
    // the float32 coefficient of one term on one variable under the current settings
    double reg_coef64(const Param* p, int term) const {
        if (!(reg_terms & term) || p->reg != term) return 0.0;
        return (term == P3D_REG_WEIGHT_DECAY ? reg_wd : reg_l2) / reg_count(term);
    }
    void set_regularization(int terms, float wd, float l2) {
        if (terms & ~(P3D_REG_WEIGHT_DECAY | P3D_REG_L2))
            throw P3dError("regularisation terms are a mask of 1 (weight decay) and 2 (l2), not " + std::to_string(terms));
        if ((terms & P3D_REG_L2) && reg_count(P3D_REG_L2) == 0)
            throw P3dError("l2: this net has no kernel_regularizer variables under scope P3D (only gn_p3d_decoder has); the "
                           "reference's mean over an empty collection is NaN");
        if ((terms & P3D_REG_WEIGHT_DECAY) && reg_count(P3D_REG_WEIGHT_DECAY) == 0) throw P3dError("weight decay: no decayed variable");
        std::vector<const Param*> tr;
        for (const Param* p : porder) if (p->trainable) tr.push_back(p);
        std::sort(tr.begin(), tr.end(), [](const Param* a, const Param* b) { return a->off < b->off; });
        const int saved = reg_terms;
        reg_terms = terms;
        reg_wd = wd > 0.f ? (double)wd : (gn_net() ? 0.0005 : 0.001);
        reg_l2 = l2 > 0.f ? (double)l2 : 0.0005;
        std::vector<P3dRegTile> tiles;
        auto cut = [&](int64_t a, int64_t b, float c) {
            for (; a < b; a += REG_TILE) tiles.push_back({(long long)a, (int)std::min(REG_TILE, b - a), c});
        };
        for (size_t i = 0; i < tr.size(); ++i) {
            const int64_t end = i + 1 < tr.size() ? tr[i + 1]->off : n_train;
            const float c = (float)(reg_coef64(tr[i], P3D_REG_WEIGHT_DECAY) + reg_coef64(tr[i], P3D_REG_L2));
            if (!tr[i]->reg) { cut(tr[i]->off, end, 0.f); continue; }      // (the cut does not depend on the settings)
            cut(tr[i]->off, tr[i]->off + tr[i]->count, c);
            cut(tr[i]->off + tr[i]->count, end, 0.f);
        }
        if (tiles.empty() || tiles[0].off != 0) { reg_terms = saved; throw P3dError("regularisation: no trainable variable at offset 0"); }
        HIPCHECK(hipStreamSynchronize(stream));      // the table may be in use by queued work
        if (!d_reg_tiles) {
            d_reg_tiles = dalloc<P3dRegTile>((int64_t)tiles.size());
            d_reg_part = dalloc<double>((int64_t)tiles.size());
            d_reg = dalloc<double>(1);
            d_reg_cnt = dalloc<unsigned>(1);
            HIPCHECK(fill_async(d_reg, 0, sizeof(double), stream, "regularisation"));
            HIPCHECK(fill_async(d_reg_cnt, 0, sizeof(unsigned), stream, "regularisation"));
        }
        HIPCHECK(copy_now(d_reg_tiles, tiles.data(), tiles.size() * sizeof(P3dRegTile), hipMemcpyHostToDevice, stream));
        reg_tiles = std::move(tiles);
        reg_decayed.assign(reg_tiles.size() + 1, 0);
        for (size_t k = 0; k < reg_tiles.size(); ++k) reg_decayed[k + 1] = reg_decayed[k] + (reg_tiles[k].c != 0.f ? reg_tiles[k].len : 0);
        if (clip_on()) build_clip_table();      // its chunks carry these coefficients
        drop_step_graph();
    }
    // adam_range's launch, from the handle: P3D_OPT_* are the UPD_* of p3d_kernels.h; with a term on, the tiles of [lo, hi), which
    // must start and end on tile boundaries, and *decayed = its elements with c != 0.
    OptArgs opt_args(int64_t lo, int64_t hi, bool update, float lr_t, const float* lr_dev, double* decayed) const {
        OptArgs a;
        a.update = update ? opt_kind : UPD_NONE;
        a.p = flat_p + lo; a.g = flat_g + lo; a.m = flat_m + lo; a.v = flat_v + lo; a.n = (long)(hi - lo);
        a.lr = lr_t; a.lr_dev = lr_dev;
        a.b1 = b1; a.b2 = b2; a.eps = eps; a.momentum = momentum; a.nesterov = use_nesterov;
        if (update && clip_on()) a.gscale = clip_scale_dev();
        if (!reg_terms) return a;
        auto at = [&](int64_t off) {
            return (int)(std::lower_bound(reg_tiles.begin(), reg_tiles.end(), off,
                                          [](const P3dRegTile& t, int64_t o) { return t.off < o; }) - reg_tiles.begin());
        };
        const int t0 = at(lo), t1 = at(hi);
        if (t0 >= (int)reg_tiles.size() || reg_tiles[t0].off != lo || t1 <= t0 || reg_tiles[t1 - 1].off + reg_tiles[t1 - 1].len != hi)
            throw P3dError("regularisation: range is not on tile boundaries");
        *decayed = (double)(reg_decayed[t1] - reg_decayed[t0]);
        a.tiles = d_reg_tiles + t0; a.ntile = t1 - t0; a.tile_base = lo;
        a.part = d_reg_part + t0; a.fold_part = d_reg_part; a.nfold = lo == 0 ? (int)reg_tiles.size() : 0;
        a.counter = d_reg_cnt; a.term = d_reg;
        return a;
    }
    double read_regularization() {
        double r = 0.0;
        if (!reg_terms) return r;
        HIPCHECK(hipMemcpyAsync(&r, d_reg, sizeof(double), hipMemcpyDeviceToHost, stream));
        HIPCHECK(hipStreamSynchronize(stream));
        return r;
    }

    // ---- captured train step (opt-in: P3D_GRAPH=1) ---------------------------------------------------
    // One train step is ~1000 dependent launches on three streams.  The launch list is static, so it CAN be captured
    // once into a hipGraph (per dropout rate / pointwise mode / communicator) and replayed; the two per-step scalars
    // (dropout seed, Adam's bias-corrected step size) then live in device memory and are written by a one-thread
    // kernel ahead of each replay.  Measured on MI355X / ROCm 7.2 (profiles/r02_graph_vs_eager.json): a replay costs the
    // host 17.1 ms per step against 9.2 ms of eager enqueueing, and the step takes 20.3 ms instead of 18.2 -- this
    // runtime walks a graph node by node and pays more per kernel node than per eager launch, so replay is slower
    // here.  The capture path is kept (and tested) for runtimes where that changes; eager is the default.
    hipGraph_t step_graph = nullptr;
    hipGraphExec_t step_exec = nullptr;
    float graph_drop = -1.f; bool graph_f16 = false; ncclComm_t graph_comm = nullptr; float graph_b1 = 0, graph_b2 = 0, graph_eps = 0;
    int graph_reg = 0;
    float graph_clip = 0.f;
    int graph_kind = P3D_OPT_ADAM; float graph_mom = 0.f; int graph_nesterov = 0;      // the optimiser the graph launches
    bool graph_ema = false, graph_ema_warmup = false; double graph_ema_decay = 0.0;    // and the moving average
    bool graph_disabled = false;
    unsigned long long* d_seed = nullptr; float* d_lr = nullptr;
    void drop_step_graph() {
        if (step_exec) { hipGraphExecDestroy(step_exec); step_exec = nullptr; }
        if (step_graph) { hipGraphDestroy(step_graph); step_graph = nullptr; }
    }
    bool graphs_enabled() {
        return runtime_env().graph && !graph_disabled;
    }
    void capture_step_graph(float drop) {
        drop_step_graph();
        Ctx c; c.training = true; c.drop = drop; c.seed = 0; c.seed_dev = d_seed; c.lr_dev = d_lr; c.om_dev = d_om; c.update_moving = true; c.s = stream;
        HIPCHECK(hipStreamBeginCapture(stream, hipStreamCaptureModeRelaxed));
        try {
            run_forward(c);
            run_loss(c);
            if (!run_backward(c, true, true)) run_adam(c);
        } catch (...) {
            hipGraph_t g = nullptr;
            hipStreamEndCapture(stream, &g);
            if (g) hipGraphDestroy(g);
            hipGetLastError();
            throw;
        }
        HIPCHECK(hipStreamEndCapture(stream, &step_graph));
        if (const char* dot = p3d_tune_env("P3D_TUNE_GRAPH_DOT")) hipGraphDebugDotPrint(step_graph, dot, hipGraphDebugDotFlagsVerbose);      // tuning build
        HIPCHECK(hipGraphInstantiate(&step_exec, step_graph, nullptr, nullptr, 0));
        graph_drop = drop; graph_f16 = pointwise_f16; graph_comm = comm; graph_b1 = b1; graph_b2 = b2; graph_eps = eps;
        graph_reg = reg_terms;
        graph_clip = clip_norm;
        graph_kind = opt_kind; graph_mom = momentum; graph_nesterov = use_nesterov;
        graph_ema = ema_on; graph_ema_warmup = ema_warmup; graph_ema_decay = ema_decay;
    }
    void train_step_device(float drop, uint64_t seed) {
        refuse_swapped("train step");
        check_fixations(false);      // before a capture: a refusal must not cost the step graph
        // accumulation (p3d_set_grad_accum) has three launch lists per cycle and always runs the eager one
        if (!graphs_enabled() || acc_k > 1) {
            Ctx c; c.training = true; c.drop = drop; c.seed = seed; c.update_moving = true; c.s = stream;
            zero_early(c);
            run_forward(c); run_loss(c);
            if (acc_accumulating()) {
                run_backward(c, false, false);
                grad_accum_take(c);
                return;
            }
            c.acc_finish = acc_k > 1;
            if (!run_backward(c, true, true)) run_adam(c);
            acc_pending = 0;
            return;
        }
        if (!step_exec || graph_drop != drop || graph_f16 != pointwise_f16 || graph_comm != comm || graph_b1 != b1 || graph_b2 != b2 ||
            graph_eps != eps || graph_reg != reg_terms || graph_clip != clip_norm || graph_kind != opt_kind || graph_mom != momentum ||
            graph_nesterov != use_nesterov || graph_ema != ema_on || graph_ema_warmup != ema_warmup || graph_ema_decay != ema_decay) {
            try {
                capture_step_graph(drop);
            } catch (const std::exception& e) {
                // a runtime that cannot capture this launch list (e.g. a collective that refuses capture) still trains
                fprintf(stderr, "[p3d] step graph capture failed (%s); using the eager launch list\n", e.what());
                graph_disabled = true;
                drop_step_graph();
                train_step_device(drop, seed);
                return;
            }
        }
        ++step;
        last_loss_kind = loss_kind;
        HIPCHECK(p3d_set_step_scalars(d_seed, d_lr, ema_on && ema_warmup ? d_om : nullptr, seed, opt_step_size(step), ema_om(step), stream));
        HIPCHECK(hipGraphLaunch(step_exec, stream));
    }

    void upload(const float* x, const float* y) {
        if (x) HIPCHECK(hipMemcpyAsync(x_in->p, x, (size_t)x_in->rows() * 3 * sizeof(float), hipMemcpyHostToDevice, stream));
        if (y) HIPCHECK(hipMemcpyAsync(d_y, y, (size_t)pred->rows() * sizeof(float), hipMemcpyHostToDevice, stream));
    }
    void upload_fixations(const unsigned char* fix) {
        if (!d_fix) d_fix = dalloc<unsigned char>(pred->rows());      // address stable from here on: captured steps name it
        HIPCHECK(hipMemcpyAsync(d_fix, fix, (size_t)pred->rows(), hipMemcpyHostToDevice, stream));
        fix_fresh = true;
    }
    float read_loss() {      // the data loss, plus the regularisation term when one is on
        double l = 0, r = 0;
        HIPCHECK(hipMemcpyAsync(&l, d_loss, sizeof(double), hipMemcpyDeviceToHost, stream));
        if (reg_terms) HIPCHECK(hipMemcpyAsync(&r, d_reg, sizeof(double), hipMemcpyDeviceToHost, stream));
        HIPCHECK(hipStreamSynchronize(stream));
        return reg_terms ? (float)(l + r) : (float)l;
    }
    void download_act(Act* a, float* host) {
        if (a->ld == a->C)
            HIPCHECK(hipMemcpyAsync(host, a->p, (size_t)a->rows() * a->C * sizeof(float), hipMemcpyDeviceToHost, stream));
        else
            HIPCHECK(hipMemcpy2DAsync(host, (size_t)a->C * 4, a->p, (size_t)a->ld * 4, (size_t)a->C * 4, (size_t)a->rows(),
                                      hipMemcpyDeviceToHost, stream));
        HIPCHECK(hipStreamSynchronize(stream));
    }

    ~p3d_handle() {
        drop_step_graph();
        if (comm) ncclCommDestroy(comm);
        if (ev_bucket) hipEventDestroy(ev_bucket);
        if (ev_comm_done) hipEventDestroy(ev_comm_done);
        for (hipEvent_t e : fork_events) hipEventDestroy(e);
        for (hipEvent_t e : wq_events) hipEventDestroy(e);
        if (ev_zeroed) hipEventDestroy(ev_zeroed);
        if (ev_zero_fork) hipEventDestroy(ev_zero_fork);
        if (ev_side_done) hipEventDestroy(ev_side_done);
        if (ev_side_early) hipEventDestroy(ev_side_early);
        if (ev_comm_early) hipEventDestroy(ev_comm_early);
        if (ev_side_bucket) hipEventDestroy(ev_side_bucket);
        // The facilities (video, training set, priors, fixation pool, eval-extra, the timing events) are members that own what they
        // took: their destructors run after this body, hence after the sweep of `allocs` and the return of the streams.  Every
        // path into p3d_destroy has synchronised the device, and so has p3d_create's failure path, so the order among the frees is
        // not observable.  Nothing is freed by name here: a facility that needs a line in this list is missing an owner.
        // the streams go back to the pool (net.hip, "stream pool"); every path here has synchronised the device or never launched
        if (side_stream) { if (side_pooled) give_stream(cfg.device, 1, side_stream); else hipStreamDestroy(side_stream); }
        for (void* p : allocs) hipFree(p);
        give_stream(cfg.device, 0, comm_stream);
        give_stream(cfg.device, 0, stream);
    }
