// part of net.hip (members of p3d_handle): what happens once, after the graph is built -- flat parameter / gradient buffers, which op
// owns which variable's gradient (the all-reduce buckets follow from it), plans, zero-fill arenas.
    void finalize_build() {
        flat_p = dalloc<float>(n_train); flat_g = dalloc<float>(n_train);
        flat_m = dalloc<float>(n_train); flat_v = dalloc<float>(n_train);
        flat_state = dalloc<float>(n_state);
        for (float* buf : {flat_p, flat_g, flat_m, flat_v}) HIPCHECK(fill_async(buf, 0, (size_t)n_train * 4, stream, "flat-buffer"));
        HIPCHECK(fill_now(flat_state, 0, (size_t)n_state * 4, stream));
        for (Param* p : porder) {
            if (p->trainable) { p->p = flat_p + p->off; p->g = flat_g + p->off; }
            else p->p = flat_state + p->off;
        }
        stats_arena = dalloc<double>(stats_count);
        statpart_arena = dalloc<float>(statpart_count);
        d_seed = dalloc<unsigned long long>(1);
        d_lr = dalloc<float>(1);
        d_om = dalloc<float>(1);
        red_arena = dalloc<double>(red_count);
        bnbuf = dalloc<float>(bnbuf_count);
        for (auto& f : late_bind) f();
        late_bind.clear();
        index_gradient_owners();
        for (int i = 0; i < (int)ops.size(); ++i)              // last op of the encoder's last bottleneck (ops are named blockN/...)
            if (ops[i].name.compare(0, 5, "block") == 0) defer_release_op = i;
        if (defer_release_op == (int)ops.size() - 1) defer_release_op = -1;
        // the encoder's last stage leaves CUs idle only while its tensors are small (784 rows at 8 clips of 16x112x112); the
        // budget is the decoder filter-gradient work of the unet at that size (124 GFLOP), measured to be absorbed
        defer_budget = 0;
        if (!blocks.empty()) {
            const Act* last = blocks.rbegin()->second.out;
            if (last && last->rows() <= 2048) defer_budget = 130e9;
            if (const char* e = p3d_tune_env("P3D_TUNE_DEFER_GFLOP")) defer_budget = atof(e) * 1e9;      // A/B runs
        }
        tune_plans();
        plan_zero_arenas();
    }

    // Bucketed all-reduce needs to know, after the backward of op i, the lowest flat offset above which every
    // gradient is final.  Variables are laid out in TF creation order, which need not be op order (the unet++
    // head creates its layers in the reference's order but runs them in a concat-safe order), so index the
    // owners: own_sorted = (offset, op index) ascending by offset, own_sufmin[p] = min op index over [p, end).
    std::vector<std::pair<int64_t, int>> own_sorted;
    std::vector<int> own_sufmin;
    void index_gradient_owners() {
        std::map<const Param*, int> owner;
        for (size_t i = 0; i < ops.size(); ++i)
            for (Param* p : ops[i].owns) {
                if (!p || !p->trainable) continue;
                if (owner.count(p)) throw P3dError("variable " + p->name + " has two gradient producers");
                owner[p] = (int)i;
            }
        for (Param* p : porder)
            if (p->trainable && !owner.count(p)) throw P3dError("variable " + p->name + " has no gradient producer");
        own_sorted.clear();
        for (auto& kv : owner) own_sorted.push_back({kv.first->off, kv.second});
        std::sort(own_sorted.begin(), own_sorted.end());
        own_sufmin.assign(own_sorted.size(), 0);
        int m = (int)ops.size();
        for (size_t p = own_sorted.size(); p-- > 0;) { m = std::min(m, own_sorted[p].second); own_sufmin[p] = m; }
        // brute-force check of the walk run_backward does: after op i, nothing at or above `lo` may belong to an
        // op that has not run its backward yet (a premature all-reduce would silently drop gradient terms)
        size_t pos = own_sorted.size();
        for (int i = (int)ops.size() - 1; i >= 0; --i) {
            while (pos > 0 && own_sufmin[pos - 1] >= i) --pos;
            const int64_t lo = pos < own_sorted.size() ? own_sorted[pos].first : n_train;
            for (auto& kv : owner)
                if (kv.first->off >= lo && kv.second < i)
                    throw P3dError("gradient bucket order broken at op " + ops[i].name + " / variable " + kv.first->name);
        }
        if (pos != 0) throw P3dError("gradient bucket walk does not reach offset 0");
        // split point of the two-part optimiser step (run_backward): the lowest offset above which no variable belongs to op 0
        // and none is read by op 0's backward -- the first part updates its range while that backward (the stem's filter
        // gradient, which reads the stem BatchNorm's gamma when it takes the apply pass) still runs on the side stream;
        // usable when it is 16-byte aligned and op 0 (the stem conv) really owns something below it
        adam_split = 0;
        size_t q = own_sorted.size();
        while (q > 0 && own_sufmin[q - 1] >= 1) --q;
        int64_t read_end = 0;
        for (auto& a : acts)
            if (a.stem_link)
                for (const Param* p : a.stem_link->reads) read_end = std::max(read_end, p->off + p->count);
        while (q < own_sorted.size() && own_sorted[q].first < read_end) ++q;
        if (q > 0 && q < own_sorted.size() && (own_sorted[q].first & 3) == 0) adam_split = own_sorted[q].first;
    }

    // One forward + backward over whatever the buffers hold: sizes the per-stream scratch of the K-sliced launches
    // and sets the kernels' function attributes, so that nothing allocates later (a captured step graph must not).
    // Parameters and moving statistics are not touched.
    void tune_plans() {
        Ctx c; c.training = true; c.s = stream;
        const bool want = fuse_bn;
        const bool want_bwd = fuse_bn_bwd;
        for (int mode = 0; mode < 3; ++mode) {      // every launch list: BatchNorm fusion can be switched per handle later
            fuse_bn = mode >= 1; fuse_bn_bwd = mode == 2;
            run_forward(c);
            run_loss(c);
            run_backward(c, false);
        }
        fuse_bn = want; fuse_bn_bwd = want_bwd;
        HIPCHECK(hipStreamSynchronize(c.s));
        HIPCHECK(fill_async(flat_g, 0, (size_t)n_train * sizeof(float), c.s, "gradients"));
        HIPCHECK(hipStreamSynchronize(c.s));
        pred_ready = false;           // what these passes left in `pred` is no prediction of the caller's
    }

    // Dry-run forward and backward once: every dense buffer an op would zero-fill before adding into it
    // (split-K outputs, atomically scattered gradients) is moved into one contiguous arena per phase, so a
    // step issues two memsets instead of a few hundred.
    void plan_zero_arenas() {
        for (int phase = 0; phase < 2; ++phase) {
            std::vector<std::pair<float*, size_t>> reqs;
            Ctx c; c.training = true; c.s = stream; c.dry = &reqs;
            if (phase == 0) { for (auto& op : ops) op.fwd(c); }
            else { for (int i = (int)ops.size() - 1; i >= 0; --i) ops[i].bwd(c); }
            std::vector<std::pair<Act*, bool>> movers;     // (act, is_grad)
            size_t total = 0;
            for (auto& rq : reqs)
                for (auto& a : acts) {
                    if (a.parent || !a.views.empty()) continue;
                    const size_t bytes = (size_t)a.rows() * a.C * sizeof(float);
                    if (bytes != rq.second) continue;
                    const bool is_g = (a.g == rq.first), is_p = (a.p == rq.first);
                    if (!is_g && !is_p) continue;
                    movers.push_back({&a, is_g});
                    total += (bytes + 255) / 256 * 256;
                    break;
                }
            if (!total) continue;
            char* base = (char*)dalloc<char>((int64_t)total);
            size_t off = 0;
            for (auto& mv : movers) {
                float*& ptr = mv.second ? mv.first->g : mv.first->p;
                ptr = (float*)(base + off);                 // the old allocation stays owned by `allocs`
                off += ((size_t)mv.first->rows() * mv.first->C * sizeof(float) + 255) / 256 * 256;
            }
            if (phase == 0) { zf = base; zf_bytes = total; } else { zb = base; zb_bytes = total; }
        }
    }
