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
    hipEvent_t ev_aug0 = nullptr, ev_aug1 = nullptr;      // around the last augmentation's launches (p3d_last_augment_ms)
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
            HIPCHECK(hipEventCreate(&ev_aug0));
            HIPCHECK(hipEventCreate(&ev_aug1));
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
        HIPCHECK(hipEventRecord(ev_aug0, stream));
        for (int st = 0; st < p3d_augment_stages(a); ++st) HIPCHECK(p3d_augment_launch(st, a, stream));
        HIPCHECK(hipEventRecord(ev_aug1, stream));
        aug_have = true;
    }

    // ---- smoothing and normalisation of output maps (p3d_set_postprocess) ------------------------------
    // Off by default, and off nothing here runs.  The setting is three numbers: the stage itself (postprocess.hip) is issued by
    // the two users of the handle's prediction, p3d_eval_last_frames and p3d_pred_maps_u8 (net_readout.inc: post_sequence), with
    // scratch from the stream pool at first use.  No step, launch list or captured graph ever names it.
    bool post_on = false;
    p3d_postprocess post_cfg{0.f, 0, P3D_NORM_NONE};
    // the effective radius (include/p3d_hip.h, RADIUS); throws on a setting the header refuses
    static int post_radius(const p3d_postprocess& c) {
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
    static bool post_neutral(const p3d_postprocess& c) { return c.sigma == 0.f && c.radius == 0 && c.norm == P3D_NORM_NONE; }
    // the 2r + 1 weights (include/p3d_hip.h, TAPS), r >= 1
    static std::vector<float> post_taps(float sigma, int r) {
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
    void set_postprocess(const p3d_postprocess* c) {
        const p3d_postprocess neutral{0.f, 0, P3D_NORM_NONE};
        const p3d_postprocess want = c ? *c : neutral;
        post_radius(want);                     // refuses before anything changes
        post_on = !post_neutral(want);
        post_cfg = post_on ? want : neutral;
    }

    // ---- histogram matching of output maps (p3d_set_hist_match; hist_match.hip) ---------------------------
    // Off by default, and off nothing here runs.  The setting is a mode, a bin count and (P3D_MATCH_TABLE) a copy of the caller's
    // table; the stage is issued by post_sequence (net_readout.inc) between the blur and the normalisation, with scratch from the
    // stream pool at first use.  No step, launch list or captured graph ever names it.
    struct MatchCfg {
        int mode = P3D_MATCH_OFF, nb = 256;
        std::vector<double> cdf, centres;      // P3D_MATCH_TABLE: nt entries each
        bool on() const { return mode != P3D_MATCH_OFF; }
    };
    MatchCfg match_cfg;
    static void match_bins(const char* what, int nb) {
        if (nb < 2 || nb > P3D_HIST_MAX_BINS)
            throw P3dError(std::string(what) + ": nbins must be in [2, " + std::to_string(P3D_HIST_MAX_BINS) + "], not " + std::to_string(nb));
    }
    // a supplied table as the header asks for it: 2 <= nt <= P3D_HIST_MAX_BINS, finite, non-decreasing (n_tables of them)
    static void match_table(const char* what, const double* cdf, const double* centres, int nt, int n_tables = 1) {
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
    static MatchCfg match_parse(const p3d_hist_match* c) {
        MatchCfg m;
        if (!c || c->mode == P3D_MATCH_OFF) return m;
        if (c->mode != P3D_MATCH_TABLE && c->mode != P3D_MATCH_DENSITY) throw P3dError("hist_match: unknown mode " + std::to_string(c->mode));
        match_bins("hist_match", c->nbins);
        m.mode = c->mode; m.nb = c->nbins;
        if (c->mode == P3D_MATCH_TABLE) {
            match_table("hist_match", c->cdf, c->centres, c->nt);
            m.cdf.assign(c->cdf, c->cdf + c->nt);
            m.centres.assign(c->centres, c->centres + c->nt);
        }
        return m;
    }
    void set_hist_match(const p3d_hist_match* c) { match_cfg = match_parse(c); }      // (parsed first: a refusal changes nothing)

    // ---- KL divergence and information gain of the evaluation pass (p3d_set_eval_extra; metrics_full.hip) ----
    // Off by default, and off nothing here runs or exists.  The baseline, its three statistics and the scratch of their one launch
    // are private allocations (freed when the option goes off and by the destructor, not part of `allocs`): no step, launch list
    // or captured graph names them.  The values of the last p3d_eval_last_frames stay on the host until p3d_last_eval_extra.
    int extra_flags = 0, extra_H = 0, extra_W = 0;
    float* extra_base = nullptr; double* extra_bstat = nullptr;
    std::vector<float> extra_base_host;        // p3d_get_eval_extra hands the baseline back
    std::vector<double> extra_last;            // [B][2] of the last evaluation
    enum { EXTRA_NONE = 0, EXTRA_HAVE = 1, EXTRA_SHAPE = 2 };
    int extra_state = EXTRA_NONE, extra_eval_H = 0, extra_eval_W = 0;
    void eval_extra_free() {
        for (void* p : {(void*)extra_base, (void*)extra_bstat}) if (p) hipFree(p);
        extra_base = nullptr; extra_bstat = nullptr;
        extra_base_host.clear(); extra_last.clear();
        extra_flags = 0; extra_H = extra_W = 0; extra_state = EXTRA_NONE;
    }
    // what the header asks of a setting; throws before anything changes
    static void eval_extra_check(int flags, const float* baseline, int H, int W) {
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
    static void eval_extra_upload(const float* baseline, int H, int W, float* base, double* bstat, hipStream_t s,
                                  hipMemcpyKind kind = hipMemcpyHostToDevice) {
        const long long N = (long long)H * W;
        P3dFullStats3 q;
        q.maps = base; q.n_pix = N; q.n_maps = 1; q.nblk = p3d_full_blocks(N); q.out = bstat;
        HIPCHECK(hipMalloc((void**)&q.part, (size_t)q.nblk * P3D_FULL_STATS3_PARTS * sizeof(double)));
        hipError_t e = hipMalloc((void**)&q.counter, sizeof(unsigned));
        if (e == hipSuccess) e = copy_now(base, baseline, (size_t)N * sizeof(float), kind, s);
        if (e == hipSuccess) e = fill_now(q.counter, 0, sizeof(unsigned), s);
        if (e == hipSuccess) e = p3d_full_stats3(q, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        hipFree(q.part);
        if (q.counter) hipFree(q.counter);
        HIPCHECK(e);
    }
    void set_eval_extra(int flags, const float* baseline, int H, int W) {
        eval_extra_check(flags, baseline, H, W);
        float* nb = nullptr; double* ns = nullptr;
        if (baseline) {                        // the new copy first: a failure changes nothing
            try {
                HIPCHECK(hipMalloc((void**)&nb, (size_t)H * W * sizeof(float)));
                HIPCHECK(hipMalloc((void**)&ns, 3 * sizeof(double)));
                eval_extra_upload(baseline, H, W, nb, ns, stream);
            } catch (...) {
                if (nb) hipFree(nb);
                if (ns) hipFree(ns);
                throw;
            }
        }
        eval_extra_free();
        extra_flags = flags; extra_base = nb; extra_bstat = ns;
        if (baseline) { extra_H = H; extra_W = W; extra_base_host.assign(baseline, baseline + (size_t)H * W); }
    }

    // p3d_set_eval_extra_prior: set_eval_extra with the handle's prior as the baseline, copied device to device; its statistics
    // come from the same one launch
    void set_eval_extra_prior(int flags) {
        if (flags & ~(P3D_EVAL_KLDIV | P3D_EVAL_INFO_GAIN)) throw P3dError("eval_extra: unknown flags " + std::to_string(flags));
        if (!(flags & P3D_EVAL_INFO_GAIN)) throw P3dError("eval_extra: a baseline is given without P3D_EVAL_INFO_GAIN");
        if (!prior_map) throw P3dError("eval_extra: the handle has no prior (p3d_prior_finish or p3d_set_prior_map)");
        const int H = prior_H, W = prior_W;
        float* nb = nullptr; double* ns = nullptr;
        std::vector<float> host((size_t)H * W);
        try {                                  // the new copy first: a failure changes nothing
            HIPCHECK(hipMalloc((void**)&nb, host.size() * sizeof(float)));
            HIPCHECK(hipMalloc((void**)&ns, 3 * sizeof(double)));
            eval_extra_upload(prior_map, H, W, nb, ns, stream, hipMemcpyDeviceToDevice);
            HIPCHECK(copy_now(host.data(), nb, host.size() * sizeof(float), hipMemcpyDeviceToHost, stream));
        } catch (...) {
            if (nb) hipFree(nb);
            if (ns) hipFree(ns);
            throw;
        }
        eval_extra_free();
        extra_flags = flags; extra_base = nb; extra_bstat = ns; extra_H = H; extra_W = W;
        extra_base_host.swap(host);
    }

    // ---- HIP-event times of the read-out's stages --------------------------------------------------------
    // Up to three events of one call: created at once and only when `on`, destroyed with the timer, so a throw between two marks
    // leaks none.  mark(i, s) records event i on s; ms(i) is the time from event i to event i + 1, both reached.
    struct StageTimer {
        hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
        explicit StageTimer(bool on, int count) {
            for (int i = 0; on && i < count; ++i) {
                const hipError_t e = hipEventCreate(&ev[i]);
                if (e != hipSuccess) { release(); HIPCHECK(e); }
            }
        }
        StageTimer(const StageTimer&) = delete;
        StageTimer& operator=(const StageTimer&) = delete;
        ~StageTimer() { release(); }
        void release() { for (auto& e : ev) if (e) { hipEventDestroy(e); e = nullptr; } }
        void mark(int i, hipStream_t s) { if (ev[i]) HIPCHECK(hipEventRecord(ev[i], s)); }
        float ms(int i) const { float t = 0.f; HIPCHECK(hipEventElapsedTime(&t, ev[i], ev[i + 1])); return t; }
    };

    // ---- fixation priors (p3d_prior_*, p3d_set_prior_map, p3d_set_prior_stage; prior.hip) -------------------
    // Nothing exists before p3d_prior_open or p3d_set_prior_map, and off nothing here runs.  The accumulator (uint32 counts, the
    // underflow flag, a staging buffer for uploaded maps) and the finished prior map are private allocations (freed by
    // p3d_prior_close / when the map is replaced, and by the destructor; not part of `allocs`): no step, launch list or captured
    // graph names them.  The stage is issued by post_sequence (net_readout.inc) after the blur.  The operations that need that
    // sequence (finish) live in net_readout.inc.
    bool prior_is_open = false;
    int prior_kind = P3D_PRIOR_FIXATIONS, prior_acc_H = 0, prior_acc_W = 0;
    int64_t prior_n_maps = 0;
    unsigned* prior_count = nullptr; unsigned* prior_flag = nullptr;
    unsigned char* prior_staging = nullptr; size_t prior_staging_bytes = 0;
    float* prior_map = nullptr; int prior_H = 0, prior_W = 0;
    int prior_mode = P3D_PRIOR_OFF; float prior_a = 0.f;
    double prior_ms[2] = {0.0, 0.0};           // the count launches of the last p3d_prior_add; the last p3d_prior_finish's launches
    void prior_need_open(const char* what) const {
        if (!prior_is_open) throw P3dError(std::string(what) + ": no accumulator is open (p3d_prior_open)");
    }
    void prior_close() {
        for (void* p : {(void*)prior_count, (void*)prior_flag, (void*)prior_staging}) if (p) hipFree(p);
        prior_count = nullptr; prior_flag = nullptr; prior_staging = nullptr; prior_staging_bytes = 0;
        prior_is_open = false; prior_n_maps = 0; prior_acc_H = prior_acc_W = 0;
    }
    void prior_open(int H, int W, int kind) {
        if (kind != P3D_PRIOR_FIXATIONS && kind != P3D_PRIOR_BYTES) throw P3dError("prior: kind " + std::to_string(kind) + " is neither P3D_PRIOR_FIXATIONS (0) nor P3D_PRIOR_BYTES (1)");
        if (H < 1 || W < 1 || (long long)H * W > INT32_MAX / 2) throw P3dError("prior: maps are H x W bytes, 1 <= H * W <= 2^30");
        unsigned* nc = nullptr; unsigned* nf = nullptr;
        try {                                  // the new accumulator first: a failure changes nothing
            HIPCHECK(hipMalloc((void**)&nc, (size_t)H * W * sizeof(unsigned)));
            HIPCHECK(hipMalloc((void**)&nf, sizeof(unsigned)));
            HIPCHECK(fill_now(nc, 0, (size_t)H * W * sizeof(unsigned), stream));
            HIPCHECK(fill_now(nf, 0, sizeof(unsigned), stream));
        } catch (...) {
            if (nc) hipFree(nc);
            if (nf) hipFree(nf);
            throw;
        }
        prior_close();
        prior_count = nc; prior_flag = nf; prior_is_open = true; prior_kind = kind; prior_acc_H = H; prior_acc_W = W;
    }
    bool prior_underflowed() {
        unsigned f = 0;
        HIPCHECK(copy_now(&f, prior_flag, sizeof(f), hipMemcpyDeviceToHost, stream));
        return f != 0;
    }
    // maps [n][H][W] from the host, in uploads of at most 256 MB; sign +1 adds, -1 takes maps out again
    void prior_add(const unsigned char* maps, int64_t n, int sign) {
        prior_need_open("prior_add");
        if (!maps) throw P3dError("null argument");
        if (sign != 1 && sign != -1) throw P3dError("prior_add: sign must be +1 or -1, not " + std::to_string(sign));
        if (n < 1) throw P3dError("prior_add: at least one map");
        if (sign > 0 && (n > P3D_PRIOR_MAX_MAPS || prior_n_maps + n > P3D_PRIOR_MAX_MAPS))
            throw P3dError("prior_add: " + std::to_string(prior_n_maps) + " + " + std::to_string(n) + " maps exceed P3D_PRIOR_MAX_MAPS = " + std::to_string((long long)P3D_PRIOR_MAX_MAPS));
        if (sign < 0 && n > prior_n_maps)
            throw P3dError("prior_add: " + std::to_string(n) + " maps cannot leave an accumulator of " + std::to_string(prior_n_maps));
        const size_t N = (size_t)prior_acc_H * prior_acc_W;
        const int64_t per = std::max<int64_t>(1, (int64_t)(((size_t)256 << 20) / N));
        const size_t want = (size_t)std::min(n, per) * N;
        if (want > prior_staging_bytes) {
            unsigned char* p = nullptr;
            HIPCHECK(hipMalloc((void**)&p, want));
            if (prior_staging) hipFree(prior_staging);
            prior_staging = p; prior_staging_bytes = want;
        }
        StageTimer tm(true, 2);
        double ms = 0.0;
        for (int64_t done = 0; done < n; done += per) {
            const int64_t cn = std::min(per, n - done);
            PriorCountArgs a;
            a.maps = prior_staging; a.n = cn; a.n_pix = (long long)N; a.kind = prior_kind; a.sign = sign; a.count = prior_count; a.flag = prior_flag;
            HIPCHECK(copy_now(prior_staging, maps + (size_t)done * N, (size_t)cn * N, hipMemcpyHostToDevice, stream));
            tm.mark(0, stream);
            HIPCHECK(p3d_prior_count_launch(a, stream));
            tm.mark(1, stream);
            HIPCHECK(hipStreamSynchronize(stream));
            ms += tm.ms(0);
            prior_n_maps += sign * cn;
        }
        prior_ms[0] = ms;
    }
    // a prior as the header asks for it: finite, not constant, 1 <= H * W <= 2^30
    static void prior_map_check(const float* map, int H, int W) {
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
    void prior_map_take(float* dev, int H, int W) {      // dev: a private allocation, owned from here on
        if (prior_map) hipFree(prior_map);
        prior_map = dev; prior_H = dev ? H : 0; prior_W = dev ? W : 0;
    }
    void set_prior_map(const float* map, int H, int W) {
        if (!map) {                            // dropped; a stage that is on refuses when it next runs
            prior_map_take(nullptr, 0, 0);
            return;
        }
        prior_map_check(map, H, W);
        float* p = nullptr;
        HIPCHECK(hipMalloc((void**)&p, (size_t)H * W * sizeof(float)));
        const hipError_t e = copy_now(p, map, (size_t)H * W * sizeof(float), hipMemcpyHostToDevice, stream);
        if (e != hipSuccess) { hipFree(p); HIPCHECK(e); }
        prior_map_take(p, H, W);
    }
    static void prior_stage_check(int mode, float a) {
        if (mode != P3D_PRIOR_OFF && mode != P3D_PRIOR_MUL && mode != P3D_PRIOR_MIX) throw P3dError("prior_stage: unknown mode " + std::to_string(mode));
        if (mode != P3D_PRIOR_OFF && !(a >= 0.f && a <= 1.f)) throw P3dError("prior_stage: the weight must be in [0, 1]");
    }
    void set_prior_stage(int mode, float a) {
        prior_stage_check(mode, a);
        if (mode != P3D_PRIOR_OFF && !prior_map) throw P3dError("prior_stage: the handle has no prior (p3d_prior_finish or p3d_set_prior_map)");
        prior_mode = mode; prior_a = mode != P3D_PRIOR_OFF ? a : 0.f;
    }

    // ---- fixation pool and shuffled AUC in the evaluation pass (p3d_fixpool_*, p3d_eval_shuffled_*; fixpool.hip) ---------------
    // Nothing exists before p3d_fixpool_open, and while no p3d_eval_shuffled_draws has armed it an evaluation issues what it always
    // issued.  The pool (one bit per pixel and slot), its staging buffer and the union's buffers of one batch are private
    // allocations (freed by p3d_fixpool_close and the destructor; not part of `allocs`): no step, launch list or captured graph
    // names them.  The host keeps which slots are filled.  The evaluation's part (select, clean moments, borji) is issued by
    // eval_maps (net_readout.inc).
    bool fp_is_open = false;
    int fp_H = 0, fp_W = 0;
    int64_t fp_cap = 0, fp_nw = 0;
    unsigned long long* fp_words = nullptr;
    std::vector<char> fp_filled;
    unsigned char* fp_staging = nullptr; size_t fp_staging_bytes = 0;
    double fp_pack_ms = 0.0, fp_union_ms = 0.0, fp_score_ms[2] = {0.0, 0.0};      // HIP events: last put's packs; last begin; last armed evaluation's select, moments + borji
    // one batch's union (p3d_eval_shuffled_begin) and the draws that arm the next evaluation
    int sh_B = 0, sh_M = 0; size_t sh_room = 0;
    unsigned long long* sh_uni = nullptr; unsigned* sh_prefix = nullptr; unsigned* sh_bsum = nullptr; unsigned* sh_n_other_dev = nullptr;
    unsigned* sh_counter = nullptr; int* sh_ids = nullptr;
    bool sh_begun = false, sh_armed = false, sh_have = false;
    std::vector<unsigned> sh_n_other;
    std::vector<int> sh_ranks, sh_n_rows;
    int sh_n_rep = 0; double sh_step = 0.1;
    std::vector<double> sh_last;
    void fixpool_need_open(const char* what) const {
        if (!fp_is_open) throw P3dError(std::string(what) + ": no fixation pool is open (p3d_fixpool_open)");
    }
    void shuffled_free() {
        for (void* p : {(void*)sh_uni, (void*)sh_prefix, (void*)sh_bsum, (void*)sh_n_other_dev, (void*)sh_counter, (void*)sh_ids}) if (p) hipFree(p);
        sh_uni = nullptr; sh_prefix = nullptr; sh_bsum = nullptr; sh_n_other_dev = nullptr; sh_counter = nullptr; sh_ids = nullptr;
        sh_room = 0; sh_B = sh_M = 0; sh_begun = sh_armed = sh_have = false;
    }
    void fixpool_close() {
        for (void* p : {(void*)fp_words, (void*)fp_staging}) if (p) hipFree(p);
        fp_words = nullptr; fp_staging = nullptr; fp_staging_bytes = 0; fp_filled.clear();
        fp_is_open = false; fp_H = fp_W = 0; fp_cap = fp_nw = 0;
        shuffled_free();
        vu.release();
    }
    void fixpool_open(int H, int W, int64_t capacity) {
        if (H < 1 || W < 1 || (long long)H * W > INT32_MAX / 2) throw P3dError("fixpool: maps are H x W bytes, 1 <= H * W <= 2^30");
        if (capacity < 1 || capacity > INT32_MAX) throw P3dError("fixpool: a capacity of 1 .. 2^31 - 1 maps");
        const int64_t nw = p3d_fix_words((long long)H * W);
        unsigned long long* w = nullptr;
        HIPCHECK(hipMalloc((void**)&w, (size_t)capacity * nw * sizeof(unsigned long long)));      // the new pool first: a failure changes nothing
        fixpool_close();
        fp_words = w; fp_is_open = true; fp_H = H; fp_W = W; fp_cap = capacity; fp_nw = nw;
        fp_filled.assign((size_t)capacity, 0);
    }
    // maps [n][H][W] from the host into slots first .. first + n - 1, in uploads of at most 256 MB
    void fixpool_put(int64_t first, const unsigned char* maps, int64_t n) {
        fixpool_need_open("fixpool_put");
        if (!maps) throw P3dError("null argument");
        if (n < 1 || first < 0 || first > fp_cap - n)
            throw P3dError("fixpool_put: slots " + std::to_string(first) + " .. " + std::to_string(first + n - 1) + " are not inside [0, " + std::to_string(fp_cap) + ")");
        const size_t N = (size_t)fp_H * fp_W;
        const int64_t per = std::min<int64_t>(65535, std::max<int64_t>(1, (int64_t)(((size_t)256 << 20) / N)));
        const size_t want = (size_t)std::min(n, per) * N;
        if (want > fp_staging_bytes) {
            unsigned char* p = nullptr;
            HIPCHECK(hipMalloc((void**)&p, want));
            if (fp_staging) hipFree(fp_staging);
            fp_staging = p; fp_staging_bytes = want;
        }
        StageTimer tm(true, 2);
        double ms = 0.0;
        for (int64_t done = 0; done < n; done += per) {
            const int64_t cn = std::min(per, n - done);
            FixPackArgs a;
            a.maps = fp_staging; a.n = cn; a.n_pix = (long long)N; a.words = fp_words + (first + done) * fp_nw;
            HIPCHECK(copy_now(fp_staging, maps + (size_t)done * N, (size_t)cn * N, hipMemcpyHostToDevice, stream));
            tm.mark(0, stream);
            HIPCHECK(p3d_fix_pack_launch(a, stream));
            tm.mark(1, stream);
            HIPCHECK(hipStreamSynchronize(stream));
            ms += tm.ms(0);
            std::fill(fp_filled.begin() + (first + done), fp_filled.begin() + (first + done + cn), 1);
        }
        fp_pack_ms = ms;
    }
    // ids [B][M]: every id a filled slot; 1 <= M <= 64
    void fixpool_check_ids(const char* what, const int* ids, int B, int M) const {
        fixpool_need_open(what);
        if (!ids) throw P3dError("null argument");
        if (M < 1 || M > 64) throw P3dError(std::string(what) + ": 1 .. 64 other maps per clip, not " + std::to_string(M));
        for (int b = 0; b < B; ++b)
            for (int m = 0; m < M; ++m) {
                const int id = ids[(size_t)b * M + m];
                if (id < 0 || id >= fp_cap) throw P3dError(std::string(what) + ": clip " + std::to_string(b) + ": slot " + std::to_string(id) + " is outside [0, " + std::to_string(fp_cap) + ")");
                if (!fp_filled[(size_t)id]) throw P3dError(std::string(what) + ": clip " + std::to_string(b) + ": slot " + std::to_string(id) + " was never filled (p3d_fixpool_put)");
            }
    }
    // the union, counts and scan of B rows of M slots into the handle's buffers; n_other_out [B]
    void shuffled_begin(const int* ids, int B, int M, uint32_t* n_other_out) {
        if (!n_other_out) throw P3dError("null argument");
        fixpool_check_ids("eval_shuffled_begin", ids, B, M);
        sh_begun = sh_armed = false;
        const int nsb = p3d_fix_scan_blocks(fp_nw);
        const size_t room = (size_t)B * fp_nw;
        if (room > sh_room || B > sh_B || M > sh_M) {
            const int nB = std::max(B, sh_B), nM = std::max(M, sh_M);
            const size_t nroom = std::max(room, sh_room);
            shuffled_free();
            HIPCHECK(hipMalloc((void**)&sh_uni, nroom * sizeof(unsigned long long)));
            HIPCHECK(hipMalloc((void**)&sh_prefix, nroom * sizeof(unsigned)));
            HIPCHECK(hipMalloc((void**)&sh_bsum, (size_t)nB * nsb * sizeof(unsigned)));
            HIPCHECK(hipMalloc((void**)&sh_n_other_dev, (size_t)nB * sizeof(unsigned)));
            HIPCHECK(hipMalloc((void**)&sh_counter, (size_t)nB * sizeof(unsigned)));
            HIPCHECK(hipMalloc((void**)&sh_ids, (size_t)nB * nM * sizeof(int)));
            HIPCHECK(fill_now(sh_counter, 0, (size_t)nB * sizeof(unsigned), stream));
            sh_room = nroom; sh_B = nB; sh_M = nM;
        }
        HIPCHECK(copy_now(sh_ids, ids, (size_t)B * M * sizeof(int), hipMemcpyHostToDevice, stream));
        FixUnionArgs a;
        a.pool = fp_words; a.nw = fp_nw; a.ids = sh_ids; a.B = B; a.M = M; a.nsb = nsb;
        a.uni = sh_uni; a.prefix = sh_prefix; a.bsum = sh_bsum; a.n_other = sh_n_other_dev; a.counter = sh_counter;
        StageTimer tm(true, 2);
        tm.mark(0, stream);
        HIPCHECK(p3d_fix_union_launch(a, stream));
        tm.mark(1, stream);
        sh_n_other.assign((size_t)B, 0u);
        HIPCHECK(copy_now(sh_n_other.data(), sh_n_other_dev, (size_t)B * sizeof(unsigned), hipMemcpyDeviceToHost, stream));      // the one synchronisation
        fp_union_ms = tm.ms(0);
        std::copy(sh_n_other.begin(), sh_n_other.end(), n_other_out);
        sh_begun = true;
    }
    // ranks [sum n_rows[b]][n_rep]: refused before anything is kept when a row count or a rank exceeds the clip's n_other
    static void shuffled_check_draws(const char* what, const int* ranks, const int* n_rows, const unsigned* n_other, int B, int n_rep, double step) {
        if (!n_rows) throw P3dError("null argument");
        if (n_rep < 1 || !(step > 0.0)) throw P3dError(std::string(what) + ": n_rep >= 1 and a positive step");
        size_t at = 0;
        for (int b = 0; b < B; ++b) {
            if (n_rows[b] < 0 || (unsigned)n_rows[b] > n_other[b])
                throw P3dError(std::string(what) + ": clip " + std::to_string(b) + ": " + std::to_string(n_rows[b]) + " rows, but the union holds " + std::to_string(n_other[b]) + " fixations");
            const size_t n = (size_t)n_rows[b] * n_rep;
            if (n > 0 && !ranks) throw P3dError("null argument");
            for (size_t i = 0; i < n; ++i)
                if (ranks[at + i] < 0 || (unsigned)ranks[at + i] >= n_other[b])
                    throw P3dError(std::string(what) + ": clip " + std::to_string(b) + ": rank " + std::to_string(ranks[at + i]) + " is outside [0, " + std::to_string(n_other[b]) + ")");
            at += n;
            if (at > (size_t)INT32_MAX) throw P3dError(std::string(what) + ": too many ranks");
        }
    }
    void shuffled_draws(const int* ranks, const int* n_rows, int n_rep, double step) {
        fixpool_need_open("eval_shuffled_draws");
        if (!sh_begun) throw P3dError("eval_shuffled_draws: no union is held (p3d_eval_shuffled_begin)");
        const int B = (int)sh_n_other.size();
        sh_armed = false;
        shuffled_check_draws("eval_shuffled_draws", ranks, n_rows, sh_n_other.data(), B, n_rep, step);
        size_t n = 0;
        for (int b = 0; b < B; ++b) n += (size_t)n_rows[b] * n_rep;
        sh_ranks.assign(ranks, ranks + n);
        sh_n_rows.assign(n_rows, n_rows + B);
        sh_n_rep = n_rep; sh_step = step; sh_armed = true;
    }
    // the union p3d_video_shuffled_begin holds for p3d_video_score_auc: n frames' rows of pool slots, in buffers of its own -- the
    // evaluation pass's union above, armed or not, is neither read nor written.  Freed with the pool.
    struct VideoUnion {
        int B = 0, M = 0, n = 0; size_t room = 0; bool begun = false;
        unsigned long long* uni = nullptr; unsigned* prefix = nullptr; unsigned* bsum = nullptr; unsigned* n_other_dev = nullptr;
        unsigned* counter = nullptr; int* ids = nullptr;
        std::vector<unsigned> n_other;
        void release() {
            for (void* p : {(void*)uni, (void*)prefix, (void*)bsum, (void*)n_other_dev, (void*)counter, (void*)ids}) if (p) hipFree(p);
            *this = VideoUnion();
        }
    } vu;
    void video_shuffled_begin(const int* ids, int n, int M, uint32_t* n_other_out) {
        if (!n_other_out) throw P3dError("null argument");
        if (n < 1 || n > 65535) throw P3dError("video_shuffled_begin: 1 .. 65535 frames");
        fixpool_check_ids("video_shuffled_begin", ids, n, M);
        vu.begun = false;
        const int nsb = p3d_fix_scan_blocks(fp_nw);
        const size_t room = (size_t)n * fp_nw;
        if (room > vu.room || n > vu.B || M > vu.M) {
            const int nB = std::max(n, vu.B), nM = std::max(M, vu.M);
            const size_t nroom = std::max(room, vu.room);
            vu.release();
            HIPCHECK(hipMalloc((void**)&vu.uni, nroom * sizeof(unsigned long long)));
            HIPCHECK(hipMalloc((void**)&vu.prefix, nroom * sizeof(unsigned)));
            HIPCHECK(hipMalloc((void**)&vu.bsum, (size_t)nB * nsb * sizeof(unsigned)));
            HIPCHECK(hipMalloc((void**)&vu.n_other_dev, (size_t)nB * sizeof(unsigned)));
            HIPCHECK(hipMalloc((void**)&vu.counter, (size_t)nB * sizeof(unsigned)));
            HIPCHECK(hipMalloc((void**)&vu.ids, (size_t)nB * nM * sizeof(int)));
            HIPCHECK(fill_now(vu.counter, 0, (size_t)nB * sizeof(unsigned), stream));
            vu.room = nroom; vu.B = nB; vu.M = nM;
        }
        HIPCHECK(copy_now(vu.ids, ids, (size_t)n * M * sizeof(int), hipMemcpyHostToDevice, stream));
        FixUnionArgs a;
        a.pool = fp_words; a.nw = fp_nw; a.ids = vu.ids; a.B = n; a.M = M; a.nsb = nsb;
        a.uni = vu.uni; a.prefix = vu.prefix; a.bsum = vu.bsum; a.n_other = vu.n_other_dev; a.counter = vu.counter;
        HIPCHECK(p3d_fix_union_launch(a, stream));
        vu.n_other.assign((size_t)n, 0u);
        HIPCHECK(copy_now(vu.n_other.data(), vu.n_other_dev, (size_t)n * sizeof(unsigned), hipMemcpyDeviceToHost, stream));      // the one synchronisation
        std::copy(vu.n_other.begin(), vu.n_other.end(), n_other_out);
        vu.n = n; vu.begun = true;
    }

    // ---- resident video inference (p3d_video_*; video.hip) ---------------------------------------------
    // Nothing exists before the first p3d_video_open and nothing here runs while no video is open.  The stores are private
    // allocations (freed by p3d_video_close, not part of `allocs`): no step, launch list or captured graph names them.  The gather
    // writes the staged x_in, whose address never moves, as an upload does.  The host keeps the authoritative counts and which
    // frames were put; the device's copy of the counts follows the scatter launches.  Every entry point ends synchronised, so
    // the next call may overwrite the host tables.
    bool vid_is_open = false;
    int vid_F = 0, vid_mode = VIDEO_NEWEST, vid_last = -1;
    int64_t vid_cap = 0;                       // frames the allocation holds
    float* vid_frames = nullptr; float* vid_maps = nullptr; int32_t* vid_count_dev = nullptr;
    unsigned char* vid_u8 = nullptr; size_t vid_u8_bytes = 0;      // staging of p3d_video_put_frames_u8's bytes
    // p3d_video_keep_source: the decoded frames [F][H0][W0][3] as they were put, for p3d_video_render.  Off: nothing of it exists
    bool vid_keep = false, vid_u8_put = false;                     // vid_u8_put: a p3d_video_put_frames_u8 has run since the open
    unsigned char* vid_src = nullptr; size_t vid_src_bytes = 0;
    int vid_H0 = 0, vid_W0 = 0;
    std::vector<unsigned char> vid_has_src;                        // [F]: the frame's bytes are in the store
    P3dVideoDst* d_vid_dst = nullptr; int* d_vid_src = nullptr; int* d_vid_starts = nullptr;      // the per-call tables, [B*T], [B*T], [B]
    int* d_vid_slots = nullptr;                                    // p3d_video_predict_shots's per-call table [B*T], from its first call
    std::vector<int32_t> vid_count; std::vector<unsigned char> vid_put;
    hipEvent_t ev_vid[4] = {nullptr, nullptr, nullptr, nullptr};      // around the last call's gather and scatter (p3d_video_last_ms)
    bool vid_timed = false;
    int64_t vid_frame_elems() const { return (int64_t)x_in->H * x_in->W * 3; }
    int64_t vid_hw() const { return (int64_t)pred->H * pred->W; }

    // What one p3d_video_predict does to the stores, from host state alone (no HIP call): validates as the header says -- the
    // message names the first offending window or frame -- and builds the padded starts, the scatter table and the counts after
    // the call.  put (or null: every frame counts as put) has F entries.
    //
    // shots (or null: p3d_video_predict's plan, windows of T consecutive frames wherever they lie) is the installed table of
    // n_shots starts: the plan of p3d_video_predict_shots ("Shot-aware windows").  Window k then reads slots [k * T + t] = g(k, t),
    // reflected inside its shot, and only its first live [k] slots -- the frames starts[k] + t themselves -- reach the scatter table.
    struct VideoPlan {
        std::vector<int> starts; std::vector<P3dVideoDst> dst; std::vector<int> src; std::vector<int32_t> count;
        std::vector<int> slots, live;      // [B * T], [B]: under a shot table only; the padding clips repeat the last window's slots, live 0
    };
    static int video_refl(int j, int L) {      // the TEMPORAL paragraph's periodic reflect-101 of j >= 0 into 0 .. L - 1
        if (L == 1) return 0;
        const int m = j % (2 * L - 2);
        return m < L ? m : 2 * L - 2 - m;
    }
    static VideoPlan video_plan(int mode, int F, int T, int B, int last_start, const int32_t* count, const unsigned char* put,
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
        VideoPlan p;
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
                const int g = lo + video_refl(starts[k] - lo + t, L);
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

    void video_need_open(const char* who) const {
        if (!vid_is_open) throw P3dError(std::string(who) + ": no video is open (p3d_video_open)");
    }
    void video_range(const char* who, int first, int n) const {
        if (n < 1 || first < 0 || first > vid_F - n)
            throw P3dError(std::string(who) + ": frames " + std::to_string(first) + " .. " + std::to_string((int64_t)first + n - 1) +
                           " are outside [0, " + std::to_string(vid_F) + ")");
    }
    void video_free() {
        for (void* p : {(void*)vid_frames, (void*)vid_maps, (void*)vid_count_dev, (void*)vid_u8, (void*)d_vid_dst, (void*)d_vid_src, (void*)d_vid_starts, (void*)d_vid_slots})
            if (p) hipFree(p);
        video_source_drop();
        vid_frames = vid_maps = nullptr; vid_count_dev = nullptr; vid_u8 = nullptr; vid_u8_bytes = 0;
        d_vid_dst = nullptr; d_vid_src = nullptr; d_vid_starts = nullptr; d_vid_slots = nullptr;
        vid_cap = 0;
    }
    // the source store goes with the video it belongs to
    void video_source_drop() {
        if (vid_src) hipFree(vid_src);
        vid_src = nullptr; vid_src_bytes = 0; vid_H0 = vid_W0 = 0; vid_keep = false; vid_u8_put = false;
        vid_has_src.clear();
    }
    void video_keep_source(int on) {
        video_need_open("video_keep_source");
        if (vid_u8_put) throw P3dError("video_keep_source: frames were already put with p3d_video_put_frames_u8; set it right after p3d_video_open");
        vid_keep = on != 0;
    }
    void video_open(int frames, int mode) {
        const int T = x_in->D, B = x_in->N;
        if (mode != VIDEO_NEWEST && mode != VIDEO_MEAN) throw P3dError("video_open: mode " + std::to_string(mode) + " is neither P3D_VIDEO_NEWEST (0) nor P3D_VIDEO_MEAN (1)");
        if (frames < T) throw P3dError("video_open: " + std::to_string(frames) + " frames, a window needs " + std::to_string(T));
        if ((int64_t)frames > INT64_MAX / 4 / vid_frame_elems()) throw P3dError("video_open: the frame store is not addressable");
        sync_streams();
        if (frames > vid_cap) {      // the new stores first: a failed allocation changes nothing
            float *nf = nullptr, *nm = nullptr; int32_t* nc = nullptr;
            const hipError_t e0 = hipMalloc((void**)&nf, (size_t)frames * vid_frame_elems() * 4);
            const hipError_t e1 = e0 == hipSuccess ? hipMalloc((void**)&nm, (size_t)frames * vid_hw() * 4) : e0;
            const hipError_t e2 = e1 == hipSuccess ? hipMalloc((void**)&nc, (size_t)frames * 4) : e1;
            if (e2 != hipSuccess) {
                if (nf) hipFree(nf);
                if (nm) hipFree(nm);
                (void)hipGetLastError();
                throw P3dError("video_open: no device memory for " + std::to_string(frames) + " frames (" + hipGetErrorString(e2) + ")");
            }
            for (void* p : {(void*)vid_frames, (void*)vid_maps, (void*)vid_count_dev}) if (p) hipFree(p);
            vid_frames = nf; vid_maps = nm; vid_count_dev = nc; vid_cap = frames;
        }
        if (!d_vid_dst) {
            HIPCHECK(hipMalloc((void**)&d_vid_dst, (size_t)B * T * sizeof(P3dVideoDst)));
            HIPCHECK(hipMalloc((void**)&d_vid_src, (size_t)B * T * sizeof(int)));
            HIPCHECK(hipMalloc((void**)&d_vid_starts, (size_t)B * sizeof(int)));
        }
        if (!ev_vid[0]) for (auto& e : ev_vid) HIPCHECK(hipEventCreate(&e));
        HIPCHECK(fill_now(vid_count_dev, 0, (size_t)frames * 4, stream));
        vid_count.assign((size_t)frames, 0);
        vid_put.assign((size_t)frames, 0);
        video_source_drop();
        vid_shots.clear();
        vid_F = frames; vid_mode = mode; vid_last = -1; vid_is_open = true; vid_timed = false;
    }
    void video_close() {
        sync_streams();
        video_free();
        vid_count.clear(); vid_put.clear(); vid_shots.clear();
        vid_is_open = false; vid_F = 0; vid_last = -1; vid_timed = false;
    }
    void video_put_frames(int first, const float* x, int n) {
        video_need_open("video_put_frames");
        video_range("video_put_frames", first, n);
        HIPCHECK(copy_now(vid_frames + (int64_t)first * vid_frame_elems(), x, (size_t)n * vid_frame_elems() * 4, hipMemcpyHostToDevice, stream));
        std::fill(vid_put.begin() + first, vid_put.begin() + first + n, (unsigned char)1);
        if (!vid_has_src.empty()) std::fill(vid_has_src.begin() + first, vid_has_src.begin() + first + n, (unsigned char)0);      // floats have no source
    }
    void video_put_frames_u8(int first, const unsigned char* bgr, int n, int H0, int W0, const float mean_rgb[3]) {
        video_need_open("video_put_frames_u8");
        video_range("video_put_frames_u8", first, n);
        if (H0 < 1 || W0 < 1) throw P3dError("video_put_frames_u8: empty frame");
        const size_t bytes = (size_t)n * H0 * W0 * 3;
        if (vid_keep) {      // the upload lands in the source store and the normalising launch reads it there
            const size_t frame = (size_t)H0 * W0 * 3;
            if (!vid_src) {
                unsigned char* ns = nullptr;
                const hipError_t e = hipMalloc((void**)&ns, (size_t)vid_F * frame);
                if (e != hipSuccess) {
                    (void)hipGetLastError();
                    throw P3dError("video_put_frames_u8: no device memory for the source store of " + std::to_string(vid_F) + " frames of " +
                                   std::to_string(H0) + " x " + std::to_string(W0) + " (" + hipGetErrorString(e) + ")");
                }
                vid_src = ns; vid_src_bytes = (size_t)vid_F * frame; vid_H0 = H0; vid_W0 = W0;
                vid_has_src.assign((size_t)vid_F, 0);
            } else if (H0 != vid_H0 || W0 != vid_W0) {
                throw P3dError("video_put_frames_u8: the source store holds " + std::to_string(vid_H0) + " x " + std::to_string(vid_W0) + " frames, the call puts " +
                               std::to_string(H0) + " x " + std::to_string(W0));
            }
            unsigned char* at = vid_src + (size_t)first * frame;
            HIPCHECK(hipMemcpyAsync(at, bgr, bytes, hipMemcpyHostToDevice, stream));
            HIPCHECK(p3d_mapf_frames(at, n, H0, W0, vid_frames + (int64_t)first * vid_frame_elems(), x_in->H, x_in->W, mean_rgb, stream));
            HIPCHECK(hipStreamSynchronize(stream));
            std::fill(vid_has_src.begin() + first, vid_has_src.begin() + first + n, (unsigned char)1);
        } else {
            if (bytes > vid_u8_bytes) {
                HIPCHECK(hipStreamSynchronize(stream));
                if (vid_u8) hipFree(vid_u8);
                vid_u8 = nullptr; vid_u8_bytes = 0;
                HIPCHECK(hipMalloc((void**)&vid_u8, bytes));
                vid_u8_bytes = bytes;
            }
            HIPCHECK(hipMemcpyAsync(vid_u8, bgr, bytes, hipMemcpyHostToDevice, stream));
            HIPCHECK(p3d_mapf_frames(vid_u8, n, H0, W0, vid_frames + (int64_t)first * vid_frame_elems(), x_in->H, x_in->W, mean_rgb, stream));
            HIPCHECK(hipStreamSynchronize(stream));
        }
        vid_u8_put = true;
        std::fill(vid_put.begin() + first, vid_put.begin() + first + n, (unsigned char)1);
    }
    void video_predict(const int* starts, int n_windows) {
        video_need_open("video_predict");
        const int B = x_in->N, T = x_in->D;
        const VideoPlan p = video_plan(vid_mode, vid_F, T, B, vid_last, vid_count.data(), vid_put.data(), starts, n_windows);
        video_issue(p, starts[n_windows - 1]);
    }
    // p3d_video_predict_shots: the same call with every window held inside its shot of the installed table
    void video_predict_shots(const int* starts, int n_windows) {
        video_need_open("video_predict_shots");
        if (vid_shots.empty()) throw P3dError("video_predict_shots: the open video has no shot table (p3d_video_set_shots, p3d_video_detect_shots)");
        const int B = x_in->N, T = x_in->D;
        if ((int64_t)B * T > 65535) throw P3dError("video_predict_shots: batch * T = " + std::to_string((int64_t)B * T) + " slots, the gather takes 65535");
        const VideoPlan p = video_plan(vid_mode, vid_F, T, B, vid_last, vid_count.data(), vid_put.data(), starts, n_windows, vid_shots.data(), (int)vid_shots.size());
        if (!d_vid_slots) HIPCHECK(hipMalloc((void**)&d_vid_slots, (size_t)B * T * sizeof(int)));
        video_issue(p, starts[n_windows - 1]);
    }
    // One accepted call: the tables up, gather, p3d_predict_windows's pass, scatter; a plan with slots gathers slot by slot.
    void video_issue(const VideoPlan& p, int last) {
        const int B = x_in->N, T = x_in->D;
        const bool by_slots = !p.slots.empty();
        VideoGatherArgs g;
        g.store = vid_frames; g.x = x_in->p; g.starts = d_vid_starts; g.starts_host = p.starts.data();
        g.B = B; g.T = T; g.F = vid_F; g.frame_elems = vid_frame_elems();
        VideoGatherSlotsArgs gs;
        gs.store = vid_frames; gs.x = x_in->p; gs.frames = d_vid_slots; gs.frames_host = p.slots.data();
        gs.B = B; gs.T = T; gs.F = vid_F; gs.frame_elems = vid_frame_elems();
        VideoScatterArgs sc;
        sc.mode = vid_mode; sc.pred = pred->p; sc.ld = pred->ld; sc.maps = B * T; sc.hw = vid_hw();
        sc.store = vid_maps; sc.count = vid_count_dev; sc.F = vid_F;
        sc.dst = d_vid_dst; sc.src = d_vid_src; sc.dst_host = p.dst.data(); sc.src_host = p.src.data();
        sc.ndst = (int)p.dst.size(); sc.nsrc = (int)p.src.size();
        if (by_slots) HIPCHECK(hipMemcpyAsync(d_vid_slots, p.slots.data(), p.slots.size() * sizeof(int), hipMemcpyHostToDevice, stream));
        else HIPCHECK(hipMemcpyAsync(d_vid_starts, p.starts.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, stream));
        if (sc.ndst) HIPCHECK(hipMemcpyAsync(d_vid_dst, p.dst.data(), p.dst.size() * sizeof(P3dVideoDst), hipMemcpyHostToDevice, stream));
        if (sc.ndst) HIPCHECK(hipMemcpyAsync(d_vid_src, p.src.data(), p.src.size() * sizeof(int), hipMemcpyHostToDevice, stream));
        HIPCHECK(hipEventRecord(ev_vid[0], stream));
        if (by_slots) HIPCHECK(p3d_video_gather_slots(gs, stream));
        else HIPCHECK(p3d_video_gather(g, stream));
        HIPCHECK(hipEventRecord(ev_vid[1], stream));
        Ctx c; c.training = false; c.drop = 0.f; c.update_moving = false; c.per_sample = true; c.s = stream;      // p3d_predict_windows's pass
        run_forward(c);
        if (pred->materialize && last_forward_fused) pred->materialize(stream);
        HIPCHECK(hipEventRecord(ev_vid[2], stream));
        if (sc.ndst) HIPCHECK(p3d_video_scatter(sc, stream));
        HIPCHECK(hipEventRecord(ev_vid[3], stream));
        HIPCHECK(hipStreamSynchronize(stream));
        vid_count = p.count;
        vid_last = last;
        vid_timed = true;
    }
    // frames first .. first + n - 1 as the read-out returns them: the map store itself under NEWEST; under MEAN `scratch`
    // ([n][hw], not the store) after the division launches queued here.  Refuses a frame with count 0.
    void video_need_predicted(const char* who, int first, int n) const {
        for (int f = first; f < first + n; ++f)
            if (vid_count[(size_t)f] == 0) throw P3dError(std::string(who) + ": frame " + std::to_string(f) + " has no prediction yet (count 0)");
    }
    const float* video_finalize(const char* who, int first, int n, float* scratch, hipStream_t s) {
        video_need_open(who);
        video_range(who, first, n);
        video_need_predicted(who, first, n);
        if (vid_mode == VIDEO_NEWEST) return vid_maps + (int64_t)first * vid_hw();
        for (int done = 0; done < n; done += 32768) {
            VideoMeanArgs a;
            a.sum = vid_maps + (int64_t)(first + done) * vid_hw(); a.count = vid_count_dev + first + done;
            a.out = scratch + (int64_t)done * vid_hw(); a.n = std::min(32768, n - done); a.hw = vid_hw();
            HIPCHECK(p3d_video_mean(a, s));
        }
        return scratch;
    }

    // ---- resident training set (p3d_trainset_*; trainset.hip) -------------------------------------------
    // Nothing exists before the first p3d_trainset_open and nothing here runs while no set is open.  The stores are private
    // allocations (freed by p3d_trainset_close, not part of `allocs`): no step, launch list or captured graph names them.  The
    // gather writes the staged x_in, d_y and d_fix, whose addresses never move, as the uploads do; d_fix is allocated by the first
    // gather that writes it, as by the first p3d_upload_fixations.  The host keeps which frames were put, per tensor.  Every
    // entry point ends synchronised, so the next call may overwrite the host table.
    bool ts_is_open = false;
    int ts_format = P3D_TRAINSET_FRAMES_U8, ts_flags = 0;
    float ts_mean[3] = {0.f, 0.f, 0.f};
    std::vector<int> ts_frames;                 // F_v
    std::vector<int64_t> ts_base;               // base[v] = F_0 + .. + F_{v-1}; [V + 1], the last entry the total
    void* ts_fr = nullptr; unsigned char* ts_den = nullptr; unsigned char* ts_fix = nullptr;      // the three stores
    size_t ts_fr_bytes = 0, ts_den_bytes = 0, ts_fix_bytes = 0;                                    // what the allocations hold
    unsigned char* ts_u8 = nullptr; size_t ts_u8_bytes = 0;      // staging of the puts that run a kernel
    int* d_ts_first = nullptr;                                   // the per-call table, [B]
    std::vector<int> ts_first;
    std::vector<unsigned char> ts_put[3];                        // frames, density, fixations: [total]
    hipEvent_t ev_ts[2] = {nullptr, nullptr};                    // around the last stage's launch (p3d_trainset_last_ms)
    bool ts_timed = false;
    int64_t ts_hw() const { return (int64_t)x_in->H * x_in->W; }
    int64_t ts_total() const { return ts_base.empty() ? 0 : ts_base.back(); }
    bool ts_has_fix() const { return (ts_flags & P3D_TRAINSET_FIXATIONS) != 0; }
    size_t ts_frame_bytes() const { return (size_t)ts_hw() * 3 * (ts_format == P3D_TRAINSET_FRAMES_F32 ? 4 : 1); }
    static const char* ts_unput(int t) { return t == 0 ? ", which was never put" : t == 1 ? ", whose density map was never put" : ", whose fixation map was never put"; }

    // The global first frame of every clip of a stage, from host state alone (no HIP call): validates as the header says -- the
    // message names the first offending clip or frame.  put[t] (or null: the tensor is not written by the call) has one flag per
    // frame of the concatenation.
    static std::vector<int> trainset_plan(const char* who, const std::vector<int>& frames, const std::vector<int64_t>& base, int T, int B,
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
                        throw P3dError(c + " and holds frame " + std::to_string(start[k] + i) + ts_unput(t));
            first[(size_t)k] = (int)f0;
        }
        return first;
    }

    void trainset_need_open(const char* who) const {
        if (!ts_is_open) throw P3dError(std::string(who) + ": no training set is open (p3d_trainset_open)");
    }
    // frames first .. first + n - 1 of video v -> the first one's index in the concatenation
    int64_t trainset_range(const char* who, int v, int first, int n) const {
        if (v < 0 || v >= (int)ts_frames.size())
            throw P3dError(std::string(who) + ": video " + std::to_string(v) + " is outside [0, " + std::to_string(ts_frames.size()) + ")");
        if (n < 1 || first < 0 || first > ts_frames[(size_t)v] - n)
            throw P3dError(std::string(who) + ": frames " + std::to_string(first) + " .. " + std::to_string((int64_t)first + n - 1) +
                           " are outside video " + std::to_string(v) + "'s [0, " + std::to_string(ts_frames[(size_t)v]) + ")");
        return ts_base[(size_t)v] + first;
    }
    void trainset_free() {
        for (void* p : {ts_fr, (void*)ts_den, (void*)ts_fix, (void*)ts_u8, (void*)d_ts_first}) if (p) hipFree(p);
        ts_fr = nullptr; ts_den = ts_fix = ts_u8 = nullptr; d_ts_first = nullptr;
        ts_fr_bytes = ts_den_bytes = ts_fix_bytes = ts_u8_bytes = 0;
    }
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
        // the new stores first: a failed allocation changes nothing
        void *nf = nullptr, *nd = nullptr, *nx = nullptr;
        hipError_t e = hipSuccess;
        if (fb > ts_fr_bytes) e = hipMalloc(&nf, fb);
        if (e == hipSuccess && db > ts_den_bytes) e = hipMalloc(&nd, db);
        if (e == hipSuccess && want_fix && db > ts_fix_bytes) e = hipMalloc(&nx, db);
        if (e != hipSuccess) {
            for (void* p : {nf, nd, nx}) if (p) hipFree(p);
            (void)hipGetLastError();
            throw P3dError("trainset_open: no device memory for " + std::to_string(total) + " frames (" + hipGetErrorString(e) + ")");
        }
        if (nf) { if (ts_fr) hipFree(ts_fr); ts_fr = nf; ts_fr_bytes = fb; }
        if (nd) { if (ts_den) hipFree(ts_den); ts_den = (unsigned char*)nd; ts_den_bytes = db; }
        if (nx) { if (ts_fix) hipFree(ts_fix); ts_fix = (unsigned char*)nx; ts_fix_bytes = db; }
        if (!want_fix && ts_fix) { hipFree(ts_fix); ts_fix = nullptr; ts_fix_bytes = 0; }      // the fixation store exists only for a set that has them
        if (!d_ts_first) HIPCHECK(hipMalloc((void**)&d_ts_first, (size_t)x_in->N * sizeof(int)));
        if (!ev_ts[0]) for (auto& ev : ev_ts) HIPCHECK(hipEventCreate(&ev));
        ts_frames.assign(frames, frames + n_videos);
        ts_base = base;
        for (auto& p : ts_put) p.assign((size_t)total, 0);
        ts_format = format; ts_flags = flags;
        for (int c = 0; c < 3; ++c) ts_mean[c] = mean_rgb[c];
        ts_is_open = true; ts_timed = false;
    }
    void trainset_close() {
        sync_streams();
        trainset_free();
        ts_frames.clear(); ts_base.clear();
        for (auto& p : ts_put) p.clear();
        ts_is_open = false; ts_timed = false; ts_flags = 0;
    }
    void trainset_mark(int t, int64_t at, int n) { std::fill(ts_put[t].begin() + at, ts_put[t].begin() + at + n, (unsigned char)1); }
    // the call's bytes in the staging buffer (queued on the main stream)
    const unsigned char* trainset_stage_bytes(const unsigned char* src, size_t bytes) {
        if (bytes > ts_u8_bytes) {
            HIPCHECK(hipStreamSynchronize(stream));
            if (ts_u8) hipFree(ts_u8);
            ts_u8 = nullptr; ts_u8_bytes = 0;
            HIPCHECK(hipMalloc((void**)&ts_u8, bytes));
            ts_u8_bytes = bytes;
        }
        HIPCHECK(hipMemcpyAsync(ts_u8, src, bytes, hipMemcpyHostToDevice, stream));
        return ts_u8;
    }
    void trainset_put_frames_u8(int v, int first, const unsigned char* bgr, int n, int H0, int W0) {
        trainset_need_open("trainset_put_frames_u8");
        const int64_t at = trainset_range("trainset_put_frames_u8", v, first, n);
        if (H0 < 1 || W0 < 1) throw P3dError("trainset_put_frames_u8: empty frame");
        if (ts_format == P3D_TRAINSET_FRAMES_U8) {      // the bytes as they are: the gather normalises
            if (H0 != x_in->H || W0 != x_in->W)
                throw P3dError("trainset_put_frames_u8: the set keeps 8-bit frames (P3D_TRAINSET_FRAMES_U8), which takes frames decoded at the grid's " +
                               std::to_string(x_in->H) + " x " + std::to_string(x_in->W) + ", not " + std::to_string(H0) + " x " + std::to_string(W0));
            HIPCHECK(copy_now((unsigned char*)ts_fr + (size_t)at * ts_frame_bytes(), bgr, (size_t)n * ts_frame_bytes(), hipMemcpyHostToDevice, stream));
        } else {
            const unsigned char* src = trainset_stage_bytes(bgr, (size_t)n * H0 * W0 * 3);
            HIPCHECK(p3d_mapf_frames(src, n, H0, W0, (float*)ts_fr + at * ts_hw() * 3, x_in->H, x_in->W, ts_mean, stream));
            HIPCHECK(hipStreamSynchronize(stream));
        }
        trainset_mark(0, at, n);
    }
    void trainset_put_frames(int v, int first, const float* x, int n) {
        trainset_need_open("trainset_put_frames");
        const int64_t at = trainset_range("trainset_put_frames", v, first, n);
        if (ts_format != P3D_TRAINSET_FRAMES_F32)
            throw P3dError("trainset_put_frames: the set keeps 8-bit frames (P3D_TRAINSET_FRAMES_U8); normalised floats need P3D_TRAINSET_FRAMES_F32");
        HIPCHECK(copy_now((float*)ts_fr + at * ts_hw() * 3, x, (size_t)n * ts_frame_bytes(), hipMemcpyHostToDevice, stream));
        trainset_mark(0, at, n);
    }
    void trainset_put_density_u8(int v, int first, const unsigned char* grey, int n, int H0, int W0) {
        trainset_need_open("trainset_put_density_u8");
        const int64_t at = trainset_range("trainset_put_density_u8", v, first, n);
        if (H0 < 1 || W0 < 1) throw P3dError("trainset_put_density_u8: empty map");
        const unsigned char* src = trainset_stage_bytes(grey, (size_t)n * H0 * W0);
        HIPCHECK(p3d_mapf_density_u8(src, n, H0, W0, ts_den + at * ts_hw(), x_in->H, x_in->W, stream));
        HIPCHECK(hipStreamSynchronize(stream));
        trainset_mark(1, at, n);
    }
    void trainset_put_fixations(int v, int first, const unsigned char* fix, int n) {
        trainset_need_open("trainset_put_fixations");
        const int64_t at = trainset_range("trainset_put_fixations", v, first, n);
        if (!ts_has_fix()) throw P3dError("trainset_put_fixations: the set was opened without P3D_TRAINSET_FIXATIONS");
        HIPCHECK(copy_now(ts_fix + at * ts_hw(), fix, (size_t)n * (size_t)ts_hw(), hipMemcpyHostToDevice, stream));
        trainset_mark(2, at, n);
    }
    // validates (nothing launched on a refusal), then queues the table and the one launch between the stage's events.
    // targets: x alone (p3d_trainset_forward), or x, y and -- when the set has them -- the fixations.
    void trainset_gather(const char* who, const int* video, const int* start, int n, bool targets) {
        trainset_need_open(who);
        const int B = x_in->N, T = x_in->D;
        const bool with_fix = targets && ts_has_fix();
        const unsigned char* const put[3] = {ts_put[0].data(), targets ? ts_put[1].data() : nullptr, with_fix ? ts_put[2].data() : nullptr};
        std::vector<int> first = trainset_plan(who, ts_frames, ts_base, T, B, video, start, n, put);
        if (with_fix && !d_fix) d_fix = dalloc<unsigned char>(pred->rows());      // address stable from here on: captured steps name it
        ts_first.swap(first);
        TrainsetGatherArgs a;
        a.format = ts_format == P3D_TRAINSET_FRAMES_F32 ? TRAINSET_F32 : TRAINSET_U8;
        a.frames = ts_fr; a.density = ts_den; a.fixations = ts_fix;
        a.x = x_in->p; a.y = targets ? d_y : nullptr; a.fix = with_fix ? d_fix : nullptr;
        a.first = d_ts_first; a.first_host = ts_first.data(); a.video_host = video; a.start_host = start;
        a.frames_host = ts_frames.data(); a.n_videos = (int)ts_frames.size();
        a.B = B; a.T = T; a.hw = ts_hw();
        for (int c = 0; c < 3; ++c) a.mean[c] = ts_mean[c];
        HIPCHECK(hipMemcpyAsync(d_ts_first, ts_first.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, stream));
        HIPCHECK(hipEventRecord(ev_ts[0], stream));
        HIPCHECK(p3d_trainset_gather(a, stream));
        HIPCHECK(hipEventRecord(ev_ts[1], stream));
        if (with_fix) fix_fresh = true;      // the gather is the upload p3d_upload_fixations would have been
        ts_timed = true;
    }
    // p3d_trainset_step's refusals that do not depend on the clips, ahead of anything that changes state
    void trainset_step_check() const {
        trainset_need_open("trainset_step");
        refuse_swapped("train step");
        if (saliency_needs_fixations() && !ts_has_fix())
            throw P3dError("trainset_step: the loss has an NSS term (w_nss > 0) and the training set was opened without P3D_TRAINSET_FIXATIONS");
    }

    // ---- temporal smoothing of the video's maps at read-out (p3d_set_video_temporal; temporal.hip) -------
    // Off by default, and off nothing here runs.  The setting is a kind with its radius and taps, or its alpha; the stage is one
    // launch issued by the two read-outs in place of video_finalize, into scratch from the stream pool.  The events exist from the
    // first run on.  No step, launch list or captured graph ever names it.
    struct TemporalCfg {
        p3d_video_temporal set{P3D_TEMPORAL_OFF, 0.f, 0, 0.f};      // as given
        int r = 0; std::vector<float> w;                            // GAUSS: the effective radius and w_r .. w_2r
        bool on() const { return set.kind != P3D_TEMPORAL_OFF; }
    };
    TemporalCfg temporal_cfg;
    hipEvent_t ev_temporal[2] = {nullptr, nullptr};
    bool temporal_timed = false;
    // what a setting asks for (include/p3d_hip.h); throws on a setting the header refuses.  Host only.
    static TemporalCfg temporal_parse(const p3d_video_temporal* c) {
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
            const std::vector<float> taps = post_taps(c->sigma, r);
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
    static void temporal_check(const char* who, const TemporalCfg& t, int F, int first, int n, const int32_t* count) {
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
    static VideoTemporalArgs temporal_args(const TemporalCfg& t, const float* store, const int32_t* count_dev, float* out, int F, int64_t hw,
                                           int first, int n) {
        VideoTemporalArgs a;
        a.kind = t.set.kind; a.store = store; a.count = count_dev; a.out = out; a.F = F; a.hw = hw; a.first = first; a.n = n;
        a.r = t.r; a.alpha = t.set.alpha;
        for (size_t d = 0; d < t.w.size() && d <= (size_t)TEMPORAL_MAX_RADIUS; ++d) a.w[d] = t.w[d];
        return a;
    }
    // ---- the shot table of the open video (p3d_video_set_shots, p3d_video_detect_shots; shots.hip) -------
    // None until installed, and gone with the video it belongs to.  While one is installed the temporal stage filters inside the
    // shots (the *_shots launches of temporal.hip, from a run table that follows the filtered maps in the scratch) and
    // p3d_video_reframe smooths its track inside them; nothing else reads it.
    std::vector<int32_t> vid_shots;                        // the starts, ascending from 0; empty: no table
    std::vector<int> vid_runs;                             // the host's copy of the last run table (it outlives the asynchronous upload)
    hipEvent_t ev_shots[3] = {nullptr, nullptr, nullptr};  // around the signal and the decision of the last p3d_video_detect_shots
    bool shots_timed = false;
    // the same refusals under a shot table: the reflections stay inside a shot, so r > F - 1 is no refusal, and only frames of the
    // shots that are read are needed
    static void temporal_check_shots(const char* who, const TemporalCfg& t, int F, int first, int n, const int32_t* count,
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
    void set_video_temporal(const p3d_video_temporal* c) { temporal_cfg = temporal_parse(c); }      // (refuses before anything changes)
    void video_temporal_check(const char* who, int first, int n) const {
        video_need_open(who);
        if (!vid_shots.empty()) temporal_check_shots(who, temporal_cfg, vid_F, first, n, vid_count.data(), vid_shots.data(), (int)vid_shots.size());
        else temporal_check(who, temporal_cfg, vid_F, first, n, vid_count.data());
    }
    // floats of scratch behind the n filtered maps that the run table of a read of n frames may take: at most a run a frame and one
    // more a shot, four ints each
    size_t video_temporal_table(int n) const { return vid_shots.empty() ? 0 : (size_t)n * 8; }
    // the filtered frames first .. first + n - 1 in `scratch` [n][hw]: one launch between the stage's events
    const float* video_temporal(const char* who, int first, int n, float* scratch, hipStream_t s) {
        video_temporal_check(who, first, n);
        if (!ev_temporal[0]) for (auto& e : ev_temporal) HIPCHECK(hipEventCreate(&e));
        const VideoTemporalArgs a = temporal_args(temporal_cfg, vid_maps, vid_mode == VIDEO_MEAN ? vid_count_dev : nullptr, scratch, vid_F,
                                                  vid_hw(), first, n);
        if (!vid_shots.empty()) {
            vid_runs = p3d_video_temporal_runs(a.kind, a.r, a.hw, vid_F, first, n, vid_shots.data(), (int)vid_shots.size());
            if (vid_runs.size() > video_temporal_table(n)) throw P3dError(std::string(who) + ": the run table outgrew its scratch");
            int* table = reinterpret_cast<int*>(scratch + (size_t)n * (size_t)vid_hw());
            HIPCHECK(hipMemcpyAsync(table, vid_runs.data(), vid_runs.size() * sizeof(int), hipMemcpyHostToDevice, s));
            HIPCHECK(hipEventRecord(ev_temporal[0], s));
            HIPCHECK(p3d_video_temporal_shots_launch(a, table, (int)(vid_runs.size() / 4), s));
            HIPCHECK(hipEventRecord(ev_temporal[1], s));
            temporal_timed = true;
            return scratch;
        }
        HIPCHECK(hipEventRecord(ev_temporal[0], s));
        HIPCHECK(p3d_video_temporal_launch(a, s));
        HIPCHECK(hipEventRecord(ev_temporal[1], s));
        temporal_timed = true;
        return scratch;
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
        if (ev_aug0) hipEventDestroy(ev_aug0);
        if (ev_aug1) hipEventDestroy(ev_aug1);
        for (hipEvent_t e : ev_vid) if (e) hipEventDestroy(e);
        for (hipEvent_t e : ev_temporal) if (e) hipEventDestroy(e);
        for (hipEvent_t e : ev_shots) if (e) hipEventDestroy(e);
        video_free();
        for (hipEvent_t e : ev_ts) if (e) hipEventDestroy(e);
        trainset_free();
        eval_extra_free();
        prior_close();
        prior_map_take(nullptr, 0, 0);
        fixpool_close();
        // the streams go back to the pool (net.hip, "stream pool"); every path here has synchronised the device or never launched
        if (side_stream) { if (side_pooled) give_stream(cfg.device, 1, side_stream); else hipStreamDestroy(side_stream); }
        for (void* p : allocs) hipFree(p);
        give_stream(cfg.device, 0, comm_stream);
        give_stream(cfg.device, 0, stream);
    }
