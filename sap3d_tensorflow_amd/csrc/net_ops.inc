// part of net.hip (members of p3d_handle): the graph ops -- conv, conv3d_transpose, the normalise / ReLU / add passes, max-pool --
// each with its forward and backward launch closures.  Reference: p3d.py:10-27 (convS / convT), tf.layers.* call sites.
    // ---- graph ops ---------------------------------------------------------------------------
    // tf.nn.conv3d / tf.layers.conv3d: SAME conv, optional bias, optional BN-statistics epilogue.
    Act* conv(const std::string& opname, Act* x, Param* w, Param* bias, const int k[3], const int s[3], int Cout, BN* bn,
              const std::string& out_name, bool stem = false, bool bn_has_dropout = false, int sibling = 0,
              const ConvFuse* fuse = nullptr) {
        const ConvGeo g = make_geo(x->D, x->H, x->W, k, s);
        Act* y = new_act(out_name, x->N, g.O[0], g.O[1], g.O[2], Cout);
        if (bn && stats_target(bn, y->rows(), Cout, bn_has_dropout)) reserve_stat_parts(bn, y->rows());
        const ConvFuse cf = fuse ? *fuse : ConvFuse();
        if (cf.out_bn) { if (cf.out_bn != bn) throw P3dError("fused output BatchNorm must be the conv's own"); make_fusable(bn, y->rows()); }
        fused_gate_check(s, cf.ngate);
        char* xflag = x->g ? consume(x) : nullptr;
        const int Cin = x->C;
        const int ntap = k[0] * k[1] * k[2];
        Op op;
        op.name = opname; op.kind = stem ? "conv_stem" : (ntap == 1 ? "conv_1x1x1" : "conv_kxkxk");
        op.flops = 2.0 * y->rows() * ntap * Cin * Cout;
        op.bytes = 4.0 * (x->rows() * (double)Cin + y->rows() * (double)Cout + (double)ntap * Cin * Cout);
        op.bflops = op.flops * (x->g ? 2 : 1);
        op.bbytes = op.bytes * (x->g ? 2 : 1);
        op.owns = {w}; if (bias) op.owns.push_back(bias);
        // a fused BatchNorm's parameter gradients come out of this conv's input-gradient launch (bn_grad_fold_channel)
        if (cf.out_bn) { op.owns.push_back(cf.out_bn->gamma); op.owns.push_back(cf.out_bn->beta); }
        hipEvent_t fork_ev = new_fork_event();
        if (stem) {
            // firstconv1 (p3d.py:172) on the pipelined kernels: 4-channel, W-padded copy of the clip, kw*4 contiguous
            // floats per kernel row (elementwise.hip, "stem"); 7 taps of K = 28 instead of 49 taps of K = 3
            if (k[0] != 1 || Cin != 3 || bias) throw P3dError("stem path is for [1,kh,kw,3,C] kernels without bias");
            const StemGeo sg = stem_geo(g, x->N, Cout);
            float* x4 = dalloc<float>(sg.x4_floats);
            HIPCHECK(fill_async(x4, 0, (size_t)sg.x4_floats * sizeof(float), stream, "stem-padding"));      // (p3d_create synchronises the stream)
            float* w4 = dalloc<float>(sg.w4_floats);
            float* dw4 = dalloc<float>(sg.w4_floats);
            float* spart = sg.part_floats ? dalloc<float>(sg.part_floats) : nullptr;
            auto link = std::make_shared<StemBnLink>();
            link->enabled = sg.part_floats != 0;
            y->stem_link = link;
            op.fwd = [=](const Ctx& c) {
                stem_pack(c, sg, x->p, x4, w->p, w4);
                std::vector<IgemmArgs> v{stem_forward_args(sg, x4, w4, y->p, y->ld, nullptr)};
                StatSink sink;
                run_igemm_group(c, v, false, epilogue_sink(sink, bn, y->rows(), Cout, bn_has_dropout));
            };
            op.bwd = [=](const Ctx& c) {
                const bool through_bn = link->pending;      // the BatchNorm's backward (the op before this one) left its apply pass here
                const BnBwdArgs bnargs = link->args;
                link->pending = false;
                on_side_stream(c, fork_ev, [=](const Ctx& sc) {
                    // greedy: the last launch of the backward pass -- the main stream is done
                    stem_filter_gradient(sc, sg, x4, y->g, y->ld, dw4, w->g, nullptr, /*greedy=*/true, spart, through_bn ? &bnargs : nullptr);
                });
                if (xflag) throw P3dError("the stem input carries no gradient");
            };
            ops.push_back(op);
            return y;
        }
        const auto f16 = [=] { return ntap == 1 && pointwise_f16; };      // the fp16 option's rule: 1x1x1 convs, forward and input gradient
        // sibling = 1 / 2: first / second of two convs that read the same input (ST_B: convS and convT both read relu(bn1(.)),
        // p3d.py:65-72): the first one only prepares its launch, the second sends both out as ONE grouped launch (conv_igemm2.hip,
        // igemm2_group_kernel) -- either alone leaves most CUs idle, and forking one to the side stream costs ~10 us of cross-stream
        // latency each way
        op.fwd = [=](const Ctx& c) {
            const bool fz = c.fuse && cf.at != 0;
            if (fz) fused_prefinalize(c, cf, cf.src[0].y->rows());      // on the main stream, ahead of a fork
            // fused: the A operand is the raw output of the conv before the BatchNorm (src[0].y), normalised on the fly
            const Act* xs = fz ? cf.src[0].y : x;
            std::vector<IgemmArgs> v{igemm_conv_forward(g, x->N, xs->p, xs->ld, Cin, y->p, y->ld, Cout, w->p, bias ? bias->p : nullptr, 0)};
            IgemmArgs& a = v[0];
            StatSink sink;
            const StatSink* stats = epilogue_sink(sink, bn, y->rows(), Cout, bn_has_dropout, c.fuse && cf.out_bn);
            if (sibling && !c.dry && !fz && ntap > 0) {
                sibling_prepare(a, stats);
                if (sibling == 1) {       // first of the pair: wait for the second (a stale entry would be a third class of the next pair)
                    if (!sib_pending.empty()) throw P3dError("sibling conv " + opname + ": an earlier pair never sent its launch");
                    sib_pending.push_back(a);
                    return;
                }
                if (sib_pending.size() != 1) throw P3dError("sibling conv " + opname + " has no first sibling waiting");
                sib_pending.push_back(a);
                std::vector<IgemmArgs> pair;
                pair.swap(sib_pending);
                launch_siblings(c, pair);
                return;
            }
            if (fz) {
                const bool two = cf.at == P3D_AT_RELU2;
                const FusedBn s1 = fused_bn_desc(cf.src[0], cf.src[0].y->rows(), c);
                const FusedBn s2 = two ? fused_bn_desc(cf.src[1], cf.src[1].y->rows(), c) : FusedBn();
                fused_forward_operand(a, cf.at, s1, fwd_finalized[cf.src[0].bn], two ? cf.src[1].y->p : nullptr, two ? cf.src[1].y->ld : 0,
                                      two ? &s2 : nullptr, two && fwd_finalized[cf.src[1].bn]);
            }
            if (f16()) a.f16 = 1;
            run_igemm_group(c, v, false, stats);
        };
        // The filter-gradient arguments.  fin: the normalised input of a FUSED forward was never stored; the filter gradient reads
        // it as relu(scale*y + shift) on its operand path (scale / shift published by the forward)
        const auto wgrad_args = [=](bool fin) {
            const Act* xs = fin ? cf.src[0].y : x;
            WgradArgs wa = wgrad_conv(g, x->N, xs->p, xs->ld, Cin, y->g, y->ld, Cout, w->g, bias ? bias->g : nullptr);
            if (fin) {
                const bool two = cf.at == P3D_AT_RELU2;
                fused_wgrad_x(wa, two ? 2 : 1, cf.src[0].bn->scale, cf.src[0].bn->shift, two ? cf.src[1].y->p : nullptr, two ? cf.src[1].y->ld : 0,
                              two ? cf.src[1].bn->scale : nullptr, two ? cf.src[1].bn->shift : nullptr);
            }
            return wa;
        };
        op.bwd = [=](const Ctx& c) {
            if (!(c.fuse_bwd && cf.any())) {
                // BatchNorm's backward as launches of its own (possibly after a fused forward)
                queue_wgrad(c, wgrad_args(c.fuse && cf.at != 0));
                if (xflag) {
                    const int accum = *xflag;
                    auto v = igemm_conv_input_side(g, x->N, y->g, y->ld, Cout, x->g, x->ld, Cin, w->p, nullptr, accum,
                                                   /*include_empty=*/!accum);
                    if (f16()) for (auto& a : v) a.f16 = 1;
                    run_igemm_group(c, v, accum != 0, nullptr);
                }
                return;
            }
            // ---- fused BatchNorm: y->g holds the GATED gradient of relu(bn(y)) (written by the consumer's input-gradient
            //      launch), BatchNorm's own backward happens on the operand paths below
            WgradArgs wa = wgrad_args(cf.at != 0);
            if (cf.out_bn) fused_wgrad_dy(wa, y->p, y->ld, cf.out_bn->coef);
            if (!xflag) throw P3dError("a conv with a fused BatchNorm needs an input gradient launch (it publishes the coefficients)");
            if (cf.out_bn && !c.dry) grad_finalized[cf.out_bn] = fused_bn_grad_prefinalize(c, fused_grad_desc(cf.out_bn, y->rows()));
            // where the input gradient goes: plain inputs and ungated launches write / add to x->g; gated launches send the
            // gated result to the gate's own buffers and use x->g (or cf.raw) for raw partial results only
            float* py = x->g; int pld = x->ld; int accum = *xflag;
            if (cf.ngate) {
                accum = cf.accum_in ? (int)*xflag : 0;
                if (cf.raw) { py = cf.raw->g; pld = cf.raw->ld; accum = *cf.raw_flag; }
            }
            auto v = igemm_conv_input_side(g, x->N, y->g, y->ld, Cout, py, pld, Cin, w->p, nullptr, accum, /*include_empty=*/!accum);
            bool first = true;
            for (auto& a : v) {
                if (f16()) a.f16 = 1;
                if (cf.out_bn) fused_grad_operand(a, y->p, y->ld, fused_grad_desc(cf.out_bn, y->rows()), grad_finalized[cf.out_bn], first);
                first = false;
            }
            if (cf.ngate) {
                BnGate gates[2];
                for (int q = 0; q < cf.ngate; ++q) gates[q] = bn_gate(cf.gate[q]);
                const int mt = fused_gated_epilogue(v, cf.ngate, gates, cf.raw != nullptr, !c.dry);
                for (int q = 0; q < cf.ngate && !c.dry; ++q) {
                    if (mt > cf.gate[q].bn->gpart_cap) throw P3dError("gradient partials overflow their arena slot");
                    cf.gate[q].bn->gnparts = mt;
                }
            }
            run_igemm_group(c, v, accum != 0, nullptr);
            queue_wgrad(c, wa);      // after the input gradient: its block 0 published the coefficients this one reads
        };
        ops.push_back(op);
        return y;
    }

    // tf.layers.conv3d_transpose(x, filters, k, s, 'same'): kernel [kd,kh,kw,Cout,Cin].
    Act* deconv(const std::string& opname, Act* x, Param* kern, Param* bias, const int k[3], const int s[3], int Cout, BN* bn,
                const std::string& out_name, bool bn_has_dropout = false) {
        const ConvGeo g = make_geo(x->D * s[0], x->H * s[1], x->W * s[2], k, s);    // conv whose input is y
        Act* y = new_act(out_name, x->N, g.I[0], g.I[1], g.I[2], Cout);
        if (bn && stats_target(bn, y->rows(), Cout, bn_has_dropout)) reserve_stat_parts(bn, y->rows());
        char* xflag = x->g ? consume(x) : nullptr;
        const int Cin = x->C;
        Op op;
        op.name = opname; op.kind = "deconv";
        double taps_eff = 1;
        for (int a = 0; a < 3; ++a) taps_eff *= (double)k[a] / s[a];
        op.flops = 2.0 * y->rows() * taps_eff * Cin * Cout;
        op.bytes = 4.0 * (x->rows() * (double)Cin + y->rows() * (double)Cout + (double)k[0] * k[1] * k[2] * Cin * Cout);
        op.bflops = 2 * op.flops; op.bbytes = 2 * op.bytes;
        op.owns = {kern}; if (bias) op.owns.push_back(bias);
        hipEvent_t fork_ev = new_fork_event();
        hipEvent_t class_fork = new_fork_event(), class_join = new_fork_event();
        op.fwd = [=](const Ctx& c) {
            auto v = igemm_conv_input_side(g, x->N, x->p, x->ld, Cin, y->p, y->ld, Cout, kern->p, bias ? bias->p : nullptr,
                                           0, true);
            StatSink sink;
            run_igemm_group(c, v, false, epilogue_sink(sink, bn, y->rows(), Cout, bn_has_dropout), class_fork, class_join);
        };
        op.bwd = [=](const Ctx& c) {
            // dK[tap][co][ci] = sum dy_big[o][co] * x[i][ci]  (conv wgrad with the roles of x and dy swapped)
            queue_wgrad(c, wgrad_conv(g, x->N, y->g, y->ld, Cout, x->p, x->ld, Cin, kern->g, nullptr));
            if (bias)
                on_side_stream(c, fork_ev, [=](const Ctx& sc) {
                    launch(sc, "colsum_kernel", 0, 4.0 * y->rows() * Cout, [&]() { return p3d_colsum(y->g, y->ld, y->rows(), Cout, bias->g, sc.s); });
                });
            if (xflag) {
                std::vector<IgemmArgs> v{igemm_conv_forward(g, x->N, y->g, y->ld, Cout, x->g, x->ld, Cin, kern->p, nullptr, *xflag)};
                run_igemm_group(c, v, *xflag != 0, nullptr);
            }
        };
        ops.push_back(op);
        return y;
    }

    // BN finalize + fused normalise / ReLU / add pass (modes in p3d_kernels.h) and its backward.
    // fused_site: with BatchNorm fusion on (Ctx::fuse) this pass does not run -- its consumers normalise on their operand
    // paths and the producing convs own the parameter gradients (conv(): ConvFuse); it runs when fusion is off.
    Act* bn_apply(const std::string& opname, int mode, Act* y1, BN* bn1, Act* y2, BN* bn2, Act* out, const std::string& out_name,
                  bool dropout = false, bool fused_site = false) {
        if (!out) out = new_act(out_name, y1->N, y1->D, y1->H, y1->W, y1->C);
        else if (!out_name.empty()) named[out_name] = out;
        consume(y1);                                 // y1 is a raw conv output: this op is its only consumer
        char* f2 = nullptr;
        if (y2) f2 = consume(y2);
        const bool two = (mode == 2 || mode == 3);
        const int bwd_parts = p3d_bn_bwd_parts((long)y1->rows(), y1->C);
        const int64_t red_off = statpart_count;          // backward partial sums share the (never zeroed) partials arena
        statpart_count += (two ? 2 : 1) * (int64_t)bwd_parts * 2 * y1->C;
        const int64_t coef_off = bnbuf_count;
        bnbuf_count += (two ? 4 : 2) * (int64_t)y1->C;
        const int64_t M = y1->rows();
        const int C = y1->C;
        if (mode == 0 && y1->stem_link) y1->stem_link->reads = {bn1->gamma};      // read by the stem's filter gradient (below)
        Op op;
        op.name = opname; op.kind = "bn_apply" + std::to_string(mode);
        const double tens = (double)M * C * 4.0;
        op.flops = 0; op.bytes = tens * (y2 ? 3 : 2);
        op.bflops = 0; op.bbytes = tens * (y2 ? 7 : 5);
        // the pass on this op's tensors, with the batch flags of the last forward
        auto mk = [=](const Ctx& c) {
            BnPass p;
            p.mode = mode; p.M = M; p.C = C;
            p.y1 = y1->p; p.ld1 = y1->ld; p.z = out->p; p.ldz = out->ld; p.dz = out->g; p.lddz = out->ld; p.dy1 = y1->g; p.lddy1 = y1->ld;
            if (y2) { p.y2 = y2->p; p.ld2 = y2->ld; p.dy2 = y2->g; p.lddy2 = y2->ld; p.acc2 = *f2; }
            BN* const bn[2] = {bn1, bn2};
            for (int q = 0; q < (two ? 2 : 1); ++q) {
                p.bn[q] = bn_params(bn[q]); p.dgamma[q] = bn[q]->gamma->g; p.dbeta[q] = bn[q]->beta->g; p.batch[q] = bn[q]->used_batch;
                p.part[q] = statpart_arena + red_off + (int64_t)q * bwd_parts * 2 * C; p.coef[q] = bnbuf + coef_off + (int64_t)q * 2 * C;
            }
            p.nparts = bwd_parts;
            set_dropout(p, c, dropout);
            return p;
        };
        if (!fused_site) {
            op.owns = {bn1->gamma, bn1->beta};
            if (two) { op.owns.push_back(bn2->gamma); op.owns.push_back(bn2->beta); }
        } else {
            if (mode != 0 && mode != 3 && mode != 4) throw P3dError("only the bn -> relu passes inside a bottleneck fuse");
            // reading the (never stored) normalised tensor after a fused forward: the plain apply pass on the published tables
            out->materialize = [=](hipStream_t st) {
                if (mode == 4 && y2->materialize) y2->materialize(st);      // ST_C adds relu(bnS(yS)), itself never stored
                HIPCHECK(p3d_bn_apply(bn_apply_args(mk(Ctx())), st));
            };
        }
        const bool small = bn_is_small(M, C, dropout);
        const int R = y1->D * y1->H * y1->W;
        op.fwd = [=](const Ctx& c) {
            if (fused_site && c.fuse) return;
            if (c.per_sample && (bn1->follows_flag ? c.training : true)) {
                // B independent batch-of-1 normalisations: per-(clip, channel) statistics over D*H*W, i.e. the
                // GroupNorm machinery with one channel per group and BN's epsilon
                if (c.training || c.update_moving || dropout) throw P3dError("per-sample BatchNorm is an inference path");
                ensure_per_sample_scratch();
                auto norm = [&](BN* bn, Act* y, int slot) {
                    const int64_t nc = (int64_t)y->N * C;
                    GnParams p = gn_layout(bn->gamma->p, bn->beta->p, ps_sums + (int64_t)slot * 2 * ps_nc, ps_tab + (int64_t)slot * 4 * ps_nc,
                                           y->N, C, C);
                    p.coef = nullptr;      // a forward-only table: scale, shift, mean, invstd
                    if (!c.dry) HIPCHECK(hipMemsetAsync(p.sums, 0, (size_t)nc * 2 * sizeof(double), c.s));
                    launch(c, "gn_stats_kernel", 0, tens, [&]() { return p3d_gn_stats(y->p, y->ld, y->N, R, C, p.sums, c.s); });
                    launch(c, "gn_finalize_kernel", 0, 32.0 * nc, [&]() { return p3d_gn_finalize(p, y->N, R, 1e-3f, c.s); });
                    return p;
                };
                GnOperand o1, o2;
                o1.y = y1->p; o1.ld = y1->ld; o1.g = norm(bn1, y1, 0);
                if (y2) { o2.y = y2->p; o2.ld = y2->ld; }
                if (two) o2.g = norm(bn2, y2, 1);
                const GnApplyArgs a = gn_apply_args(mode, M, R, C, 1e-3f, o1, o2, 0, nullptr, nullptr, out->p, out->ld, nullptr, c, false);
                launch(c, "gn_apply_kernel(per-sample BN)", 0, tens * (y2 ? 3 : 2), [&]() { return p3d_gn_apply(a, c.s); });
                return;
            }
            bn1->used_batch = bn1->follows_flag ? c.training : true;
            if (two) bn2->used_batch = bn2->follows_flag ? c.training : true;
            const BnPass p = mk(c);
            const BnPath path = small ? BN_SMALL : c.dry ? BN_FINALIZE
                                      : bn_path(M, C, dropout, p.batch[0] ? p.bn[0].nparts : 0, p.batch[1] ? p.bn[1].nparts : 0, p.drop_scale);
            bn_pass_forward(c, p, path, c.update_moving);
        };
        {
            auto scope = [](const BN* bn) { const std::string& n = bn->gamma->name; return n.substr(0, n.rfind('/')); };
            op.dec_kind = "bn"; op.dec_name1 = scope(bn1); op.dec_name2 = two ? scope(bn2) : std::string(); op.dec_act = y1;
            op.gates = [=](hipStream_t st, const float* ones, float* o1, float* o2, float* scratch) {
                BnPass p = mk(Ctx());      // (dropout sites: the gate alone -- the keep pattern is the tests' own input)
                p.dz = ones; p.lddz = C; p.dy1 = o1; p.lddy1 = C; p.dy2 = o2; p.lddy2 = C; p.acc2 = 0;
                p.dgamma[0] = scratch; p.dbeta[0] = scratch + C; p.dgamma[1] = scratch + 2 * C; p.dbeta[1] = scratch + 3 * C;
                p.batch[0] = p.batch[1] = 0;
                if (small) HIPCHECK(p3d_bn_small_bwd(bn_small_args(p, false), st));
                else HIPCHECK(p3d_bn_bwd_apply(bn_bwd_args(p), st));
            };
        }
        op.bwd = [=](const Ctx& c) {
            if (fused_site && c.fuse_bwd) return;
            const BnPass p = mk(c);
            // the stem: dy is read by the conv's filter gradient only, which evaluates the apply launch on its operand (stem_wgrad.hip)
            StemBnLink* stem = y1->stem_link.get();
            const bool to_stem = stem && stem->enabled && mode == 0 && !small && !(p.drop_scale > 0.f);
            bn_pass_backward(c, p, small, to_stem ? &stem->args : nullptr);
            if (to_stem) stem->pending = true;
        };
        ops.push_back(op);
        return out;
    }

    // tf.nn.max_pool3d SAME
    Act* maxpool(const std::string& opname, Act* x, const int k[3], const int s[3], Act* out, const std::string& out_name) {
        const ConvGeo g = make_geo(x->D, x->H, x->W, k, s);
        if (!out) out = new_act(out_name, x->N, g.O[0], g.O[1], g.O[2], x->C);
        else if (!out_name.empty()) named[out_name] = out;
        char* xflag = consume(x);
        // overlapping windows (pool1): the forward keeps the arg-max tap of every output so that the backward can gather
        unsigned* idx = nullptr;
        if (!p3d_maxpool_disjoint(pool_args(g, x->N, x->C, x->ld, out->ld))) idx = (unsigned*)dalloc<float>(out->rows() * (x->C / 4));
        Op op;
        op.name = opname; op.kind = "maxpool";
        op.bytes = 4.0 * (x->rows() + out->rows()) * x->C;
        op.bbytes = 4.0 * (2.0 * x->rows() + 2.0 * out->rows()) * x->C;
        auto mk = [=]() {
            // NB: k / s are pointers into the builder's stack; only the by-value geometry is safe here
            PoolArgs a = pool_args(g, x->N, x->C, x->ld, out->ld);
            a.x = x->p; a.y = out->p; a.dy = out->g; a.dx = x->g; a.idx = idx;
            return a;
        };
        op.dec_kind = "pool"; op.dec_act = x;
        op.fwd = [=](const Ctx& c) { pool_forward(c, mk()); };
        op.bwd = [=](const Ctx& c) { pool_backward(c, mk(), *xflag); };
        ops.push_back(op);
        return out;
    }
