// part of net.hip (members of p3d_handle): GroupNorm, CBAM and the GroupNorm bottleneck / heads (gn/p3d_gn.py, utils/network.py:198-274).
    // ---- GroupNorm / CBAM variant (gn/p3d_gn.py) ---------------------------------------------------
    GN* add_gn(int C) {
        gns.emplace_back();
        GN* g = &gns.back();
        g->name = unique("group_norm");
        g->C = C; g->G = C < 32 ? C : 32; g->N = cfg.batch;
        if (C % g->G) throw P3dError("GroupNorm needs C (" + std::to_string(C) + ") to be a multiple of its 32 groups");
        g->gamma = add_param(g->name + "/gamma", {C}, true, INIT_ONES);
        g->beta = add_param(g->name + "/beta", {C}, true, INIT_ZEROS);
        const int64_t nc = (int64_t)cfg.batch * C;
        g->sums_off = stats_count; stats_count += 2 * nc;
        g->bsums_off = red_count; red_count += 2 * nc;
        g->tab_off = bnbuf_count; bnbuf_count += 7 * nc;
        return g;
    }
    GnParams gn_params(GN* g, bool bwd) {
        return gn_layout(g->gamma->p, g->beta->p, bwd ? red_arena + g->bsums_off : stats_arena + g->sums_off, bnbuf + g->tab_off,
                         g->N, g->C, g->G);
    }

    // GroupNorm + fused activation pass (modes in gn.hip).  cb != null: mode 6, y2 is the CBAM input.
    Act* gn_apply(const std::string& opname, int mode, Act* y1, GN* g1, Act* y2, GN* g2, Act* out, const std::string& out_name,
                  bool dropout = false, CbamSite* cb = nullptr) {
        if (!out) out = new_act(out_name, y1->N, y1->D, y1->H, y1->W, y1->C);
        else if (!out_name.empty()) named[out_name] = out;
        consume(y1);
        char* f2 = nullptr;
        if (y2 && mode != 6) f2 = consume(y2);
        const int64_t M = y1->rows();
        const int R = y1->D * y1->H * y1->W, C = y1->C, N = y1->N;
        const double tens = (double)M * C * 4.0;
        Op op;
        op.name = opname; op.kind = "gn_apply" + std::to_string(mode);
        op.bytes = tens * (y2 ? 4 : 3); op.bbytes = tens * (y2 ? 7 : 5);
        op.owns = {g1->gamma, g1->beta};
        if (g2) { op.owns.push_back(g2->gamma); op.owns.push_back(g2->beta); }
        auto mk = [=](const Ctx& c, bool bwd) {
            const GnOperand o1{y1->p, y1->ld, y1->g, y1->ld, gn_params(g1, bwd), g1->gamma->g, g1->beta->g};
            GnOperand o2;
            if (y2) { o2.y = y2->p; o2.ld = y2->ld; o2.dy = y2->g; o2.lddy = y2->ld; }
            if (mode == 6) { o2.dy = cb->dout; o2.lddy = C; }
            if (g2) { o2.g = gn_params(g2, bwd); o2.dgamma = g2->gamma->g; o2.dbeta = g2->beta->g; }
            const CbamArgs ca = cb ? cbam_site_args(cb) : CbamArgs();      // (its channel and spatial scales)
            return gn_apply_args(mode, M, R, C, 1e-5f, o1, o2, f2 ? *f2 : 0, ca.cs, ca.ss, out->p, out->ld, out->g, c, dropout);
        };
        // small tensors (every GroupNorm of stage 3): one launch each way, see gn.hip
        const bool small = gn_small_rule(mode, R, C, g1->G, g2 ? g2->G : 0, dropout);
        if (mode != 5) {
            // decisions of the last forward (p3d_debug_decision_*): the backward apply kernel on dz = 1 with a coefficient table
            // (k, c1, c2) = (1, 0, 0) -- what it writes is the gate itself.  scratch: 2 x [N][C][3] floats + the kernel's own needs
            auto scope = [](const GN* g) { const std::string& n = g->gamma->name; return n.substr(0, n.rfind('/')); };
            op.dec_kind = "bn"; op.dec_name1 = scope(g1); op.dec_name2 = (mode == 3) ? scope(g2) : std::string(); op.dec_act = y1;
            op.dec_scratch = 6 * (int64_t)N * C + 64;
            op.gates = [=](hipStream_t st, const float* ones, float* o1, float* o2, float* scratch) {
                Ctx c; c.s = st;
                GnApplyArgs a = mk(c, true);
                std::vector<float> unit((size_t)3 * N * C);
                for (size_t i = 0; i < unit.size(); i += 3) { unit[i] = 1.f; unit[i + 1] = 0.f; unit[i + 2] = 0.f; }
                HIPCHECK(copy_now(scratch, unit.data(), unit.size() * sizeof(float), hipMemcpyHostToDevice, st));
                HIPCHECK(copy_now(scratch + unit.size(), unit.data(), unit.size() * sizeof(float), hipMemcpyHostToDevice, st));
                a.g1.coef = scratch; a.g2.coef = scratch + unit.size();
                a.dz = ones; a.ldz = C; a.drop_scale = 0.f;
                a.dy1 = o1; a.lddy1 = C; a.dy2 = o2; a.lddy2 = C; a.acc2 = 0;
                HIPCHECK(p3d_gn_bwd_apply(a, st));
            };
        }
        op.fwd = [=](const Ctx& c) { gn_pass_forward(c, mk(c, false), small); };
        op.bwd = [=](const Ctx& c) { gn_pass_backward(c, mk(c, true), small); };
        ops.push_back(op);
        return out;
    }

    CbamArgs cbam_site_args(CbamSite* cb) {
        Act* x = cb->x;
        const float* const w[5] = {cb->k0->p, cb->b0->p, cb->k1->p, cb->b1->p, cb->k7->p};
        float* const dw[5] = {cb->k0->g, cb->b0->g, cb->k1->g, cb->b1->g, cb->k7->g};
        return cbam_args(x->N, x->D, x->H, x->W, x->C, x->p, x->ld, w, cb->chunks, bnbuf + cb->buf_off, cb->dout, x->g,
                         cb->xflag ? *cb->xflag : 0, dw);
    }

    // residual = cbam_block(residual, 'cbam_<id>')  (gn/p3d_gn.py:175)
    CbamSite* cbam(Act* x, int id) {
        cbams.emplace_back();
        CbamSite* cb = &cbams.back();
        const std::string nm = "cbam_" + std::to_string(id);
        const int C = x->C, Ch = C / 8;
        if (Ch < 1) throw P3dError("CBAM needs at least 8 channels");
        cb->k0 = add_param(nm + "/ch_at/mlp_0/kernel", {C, Ch}, true, INIT_VS);
        cb->b0 = add_param(nm + "/ch_at/mlp_0/bias", {Ch}, true, INIT_ZEROS);
        cb->k1 = add_param(nm + "/ch_at/mlp_1/kernel", {Ch, C}, true, INIT_VS);
        cb->b1 = add_param(nm + "/ch_at/mlp_1/bias", {C}, true, INIT_ZEROS);
        cb->k7 = add_param(nm + "/sp_at/conv3d/kernel", {7, 7, 7, 2, 1}, true, INIT_VS);
        cb->x = x;
        cb->chunks = cbam_chunks(x->D * x->H * x->W);
        cb->dout = dalloc<float>(x->rows() * C);
        cb->buf_off = bnbuf_count; bnbuf_count += cbam_layout(x->N, x->rows(), C, cb->chunks).total;      // (net.hip)
        cb->xflag = consume(x);
        Op op;
        op.name = "block" + std::to_string(id) + "/cbam"; op.kind = "cbam";
        op.bytes = 4.0 * 2 * x->rows() * C; op.bbytes = 4.0 * 7 * x->rows() * C;
        op.owns = {cb->k0, cb->b0, cb->k1, cb->b1, cb->k7};
        op.fwd = [=](const Ctx& c) { cbam_pass_forward(c, cbam_site_args(cb)); };
        op.bwd = [=](const Ctx& c) { cbam_pass_backward(c, cbam_site_args(cb)); };
        ops.push_back(op);
        return cb;
    }

    // Bottleneck.infer of the GN file, gn/p3d_gn.py:127-179
    Act* bottleneck_gn(Act* x, int id, int inplanes, int planes, bool first, bool stride2) {
        blocks[id].in = x; blocks[id].op0 = ops.size();
        Act* r = bottleneck_gn_body(x, id, inplanes, planes, first, stride2);
        blocks[id].out = r; blocks[id].op1 = ops.size();
        return r;
    }
    Act* bottleneck_gn_body(Act* x, int id, int inplanes, int planes, bool first, bool stride2) {
        const std::string sid = std::to_string(id);
        const char st = "ABC"[id % 3];
        const int one[3] = {1, 1, 1}, s2[3] = {1, 2, 2};
        const int* s = (first && stride2) ? s2 : one;
        const int kS[3] = {1, 3, 3}, kT[3] = {3, 1, 1};
        const std::string B = "block" + sid + "/";
        Param* w1 = wd_weight("conv3_" + sid + "_1", {1, 1, 1, inplanes, planes});
        GN* g1 = add_gn(planes);
        Act* y1 = conv(B + "conv1", x, w1, nullptr, one, s, planes, nullptr, "");
        Act* z1 = gn_apply(B + "gn1", 0, y1, g1, nullptr, nullptr, nullptr, B + "conv1_bn_relu");
        const std::string nm = std::string("ST") + st + "_" + sid + "_2";
        Param* wS = wd_weight(nm + "_S", {1, 3, 3, planes, planes});
        Param* bS = conv_weight(nm + "_S_bias", {planes});
        GN* gS = add_gn(planes);
        Act* yS = conv(B + "convS", z1, wS, bS, kS, one, planes, nullptr, "");
        Act* zS = (st == 'B') ? nullptr : gn_apply(B + "gnS", 0, yS, gS, nullptr, nullptr, nullptr, "");
        Param* wT = wd_weight(nm + "_T", {3, 1, 1, planes, planes});
        Param* bT = conv_weight(nm + "_T_bias", {planes});
        GN* gT = add_gn(planes);
        Act* yT = conv(B + "convT", st == 'B' ? z1 : zS, wT, bT, kT, one, planes, nullptr, "");
        Act* stout;
        if (st == 'A') stout = gn_apply(B + "gnT", 0, yT, gT, nullptr, nullptr, nullptr, B + "st");
        else if (st == 'B') stout = gn_apply(B + "gnST", 3, yT, gT, yS, gS, nullptr, B + "st");      // relu(gn(T)) + relu(gn(S))
        else stout = gn_apply(B + "gnT", 4, yT, gT, zS, nullptr, nullptr, B + "st");
        Param* w3 = wd_weight("conv3_" + sid + "_3", {1, 1, 1, planes, planes * 4});
        GN* g3 = add_gn(planes * 4);
        Act* y3 = conv(B + "conv3", stout, w3, nullptr, one, one, planes * 4, nullptr, "");
        Act* res = x;
        if (first) {
            Param* wp = wd_weight("dw3d_" + sid, {1, 1, 1, inplanes, planes * 4});
            GN* gp = add_gn(planes * 4);
            Act* yp = conv(B + "proj", x, wp, nullptr, one, s, planes * 4, nullptr, "");
            res = gn_apply(B + "gnp", 5, yp, gp, nullptr, nullptr, nullptr, "");
        }
        CbamSite* cb = cbam(res, id);
        return gn_apply(B + "gn3", 6, y3, g3, res, nullptr, nullptr, B + "out", false, cb);
    }

    // inference_p3d, gn/p3d_gn.py:214-258
    // Stem + three GN/CBAM stages + temporal pools shared by the heads of gn/p3d_gn.py (:215-240, :491-516).
    // before_stage(stage, input) runs before the blocks of stages 1 and 2 so that a head can create its skip
    // transposed convs where the reference does (GroupNorm scopes are numbered in creation order).
    void build_gn_encoder(Act* skip2, const std::function<void(int, Act*)>& before_stage, Act* pools[3]) {
        const int B = cfg.batch, T = cfg.frames, H = cfg.height, W = cfg.width, b = cfg.base;
        if (T % 16 || H % 16 || W % 16) throw P3dError("frames/height/width must be multiples of 16");
        if (b % 8) throw P3dError("base must be a multiple of 8");
        x_in = new_act("x", B, T, H, W, 3, false);
        const int k177[3] = {1, 7, 7}, s122[3] = {1, 2, 2}, k233[3] = {2, 3, 3}, s222[3] = {2, 2, 2};
        const int k211[3] = {2, 1, 1}, s211[3] = {2, 1, 1};
        Param* w0 = wd_weight("firstconv1", {1, 7, 7, 3, b});
        GN* g0 = add_gn(b);
        Act* c1 = conv("stem/conv", x_in, w0, nullptr, k177, s122, b, nullptr, "conv1_custom", true);
        Act* a1 = gn_apply("stem/gn", 0, c1, g0, nullptr, nullptr, nullptr, "conv1_custom_bn_relu");
        Act* cur = maxpool("pool1", a1, k233, s222, nullptr, "pool1");
        int id = 0, inpl = b;
        const int planes[3] = {b, 2 * b, 4 * b};
        Act* skips[3] = {skip2, nullptr, nullptr};
        const char* pool_names[3] = {"pool2", "pool3", "pool4"};
        for (int stage = 0; stage < 3; ++stage) {
            if (stage > 0 && before_stage) before_stage(stage, cur);
            for (int j = 0; j < cfg.blocks[stage]; ++j) {
                cur = bottleneck_gn(cur, id, inpl, planes[stage], j == 0, stage > 0);
                inpl = planes[stage] * 4;
                ++id;
            }
            cur = maxpool(pool_names[stage], cur, k211, s211, skips[stage], pool_names[stage]);
            pools[stage] = cur;
        }
    }
    // tf.layers.conv3d / conv3d_transpose + GNReLU (gn/p3d_gn.py:14-22,49-51), optionally into a concat slice.  l2_layers: the
    // decoder-block head's conv3d_layers / deconv3d_layers, whose kernels carry kernel_regularizer=l2_reg() (gn/p3d_gn.py:11-21)
    bool l2_layers = false;
    Act* gn_layer(const char* name, bool up, Act* x, int filters, const int* k, const int* s, Act* out,
                  const std::string& out_name, bool dropout = false) {
        Param* kern = up ? conv_weight(std::string(name) + "/kernel", {k[0], k[1], k[2], filters, x->C})
                         : conv_weight(std::string(name) + "/kernel", {k[0], k[1], k[2], x->C, filters});
        if (l2_layers) kern->reg = P3D_REG_L2;
        Param* bi = add_param(std::string(name) + "/bias", {filters}, true, INIT_ZEROS);
        GN* g = add_gn(filters);
        Act* y = up ? deconv(name, x, kern, bi, k, s, filters, nullptr, "") : conv(name, x, kern, bi, k, s, filters, nullptr, "");
        return gn_apply(std::string(name) + "_gn", 0, y, g, nullptr, nullptr, out, out_name, dropout);
    }

    // inference_p3d (gn/p3d_gn.py:214-258; pool4_filters = 16) and inference_p3d_concat (gn/p3d_gn.py:279-324;
    // pool4_filters = 8, the only difference), filters in units of base
    void build_gn_p3d(int pool4_filters) {
        const int B = cfg.batch, T = cfg.frames, H = cfg.height, W = cfg.width, b = cfg.base;
        const int k333[3] = {3, 3, 3}, s111[3] = {1, 1, 1}, s222[3] = {2, 2, 2}, s444[3] = {4, 4, 4};
        // concatenator = [deconv_pool3_gn (8b) | deconv_pool4_gn (16b or 8b) | pool2 (4b)]  (gn/p3d_gn.py:251,317)
        const int p4 = pool4_filters * b;
        Act* cat = new_act("concatenator", B, T / 4, H / 4, W / 4, 12 * b + p4);
        Act* pools[3] = {nullptr, nullptr, nullptr};
        build_gn_encoder(new_view(cat, 8 * b + p4, 4 * b, "pool2"), [&](int stage, Act* in) {
            if (stage == 2) gn_layer("deconv_pool3", true, in, 8 * b, k333, s222, new_view(cat, 0, 8 * b, ""), "");   // before stage 3
        }, pools);
        gn_layer("deconv_pool4", true, pools[2], p4, k333, s444, new_view(cat, 8 * b, p4, ""), "");
        Act* zc = gn_layer("conv_concat", false, cat, 16 * b, k333, s111, nullptr, "conv_concat");
        Act* zr = gn_layer("deconv_revise", true, zc, 4 * b, k333, s222, nullptr, "deconv_revise", /*dropout=*/true);
        Param* kp = conv_weight("predict_revise/kernel", {3, 3, 3, 1, 4 * b});
        Param* bp = add_param("predict_revise/bias", {1}, true, INIT_ZEROS);
        head(zr, kp, bp, /*with_sigmoid=*/false);
    }

    // inference_p3d_decoder_block (gn/p3d_gn.py:489-539, net = 'P3D_DECODER' in gn/train_p3d_gn_dataset.py:177):
    // everything lives in tf.variable_scope('P3D'); skip deconvs of pool2/3/4 to 4x28x28, concat, conv_concat, two
    // conv-deconv-conv decoder blocks narrowing to base/4 channels at full resolution, dropout, and a plain
    // 3x3x3 conv to one channel (no sigmoid).
    void build_gn_decoder() {
        const int B = cfg.batch, T = cfg.frames, H = cfg.height, W = cfg.width, b = cfg.base;
        if (b % 16) throw P3dError("the decoder-block head needs base to be a multiple of 16");
        var_prefix = "P3D/";
        l2_layers = true;
        const int k333[3] = {3, 3, 3}, k233[3] = {2, 3, 3}, k133[3] = {1, 3, 3};
        const int s111[3] = {1, 1, 1}, s222[3] = {2, 2, 2}, s444[3] = {4, 4, 4};
        Act* cat = new_act("concatenator", B, T / 4, H / 4, W / 4, 14 * b);   // [deconv_pool2 2b | deconv_pool3 4b | deconv_pool4 8b]
        Act* pools[3] = {nullptr, nullptr, nullptr};
        build_gn_encoder(nullptr, [&](int stage, Act* in) {
            if (stage == 1) gn_layer("deconv_pool2", true, in, 2 * b, k333, s111, new_view(cat, 0, 2 * b, ""), "deconv_pool2");
            else gn_layer("deconv_pool3", true, in, 4 * b, k233, s222, new_view(cat, 2 * b, 4 * b, ""), "deconv_pool3");
        }, pools);
        gn_layer("deconv_pool4", true, pools[2], 8 * b, k133, s444, new_view(cat, 6 * b, 8 * b, ""), "deconv_pool4");
        Act* z = gn_layer("conv_concat", false, cat, 16 * b, k333, s111, nullptr, "conv_concat");
        z = gn_layer("decoder1_conv1", false, z, 4 * b, k333, s111, nullptr, "decoder1_conv1");
        z = gn_layer("decoder1_deconv", true, z, 4 * b, k333, s222, nullptr, "decoder1_deconv");
        z = gn_layer("decoder1_conv2", false, z, 2 * b, k333, s111, nullptr, "decoder1_conv2");
        z = gn_layer("decoder2_conv1", false, z, b / 2, k333, s111, nullptr, "decoder2_conv1");
        z = gn_layer("decoder2_deconv", true, z, b / 2, k333, s222, nullptr, "decoder2_deconv");
        z = gn_layer("decoder2_conv2", false, z, b / 4, k333, s111, nullptr, "decoder2_conv2", /*dropout=*/true);
        Param* kp = conv_weight("results/kernel", {3, 3, 3, b / 4, 1});
        kp->reg = P3D_REG_L2;                 // tf.layers.conv3d(..., kernel_regularizer=l2_reg(), name='results') (gn/p3d_gn.py:538)
        Param* bp = add_param("results/bias", {1}, true, INIT_ZEROS);
        head(z, kp, bp, /*with_sigmoid=*/false, /*transpose=*/false);
    }
