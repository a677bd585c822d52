// part of net.hip (members of p3d_handle): the reference graphs -- Bottleneck / make_block, encoder, p3d_unet, p3d_concat, the UNet++
// heads with attention(), the output head (p3d.py:30-221,226-397; utils/network.py:157-192).
    // ---- the reference graph -------------------------------------------------------------------
    Param* conv_weight(const std::string& name, std::vector<int64_t> shape) { return add_param(name, shape, true, INIT_XAVIER); }
    // get_conv_weight with wd != 0 (p3d.py:10-16, gn/p3d_gn.py:54-60): its l2_loss goes to 'weightdecay_losses'.  conv_weight()
    // also makes the convS/convT biases (wd = 0) and the head and attention kernels, which are not in that collection.
    Param* wd_weight(const std::string& name, std::vector<int64_t> shape) {
        Param* w = conv_weight(name, shape);
        w->reg = P3D_REG_WEIGHT_DECAY;
        return w;
    }

    // Bottleneck.infer, p3d.py:83-136 (3-D branch only; the 2-D branch is unreachable, SURVEY fact 7)
    // per bottleneck: input / output tensors and the [first, last) range of its ops, for p3d_block_forward
    struct BlockInfo { Act* in = nullptr; Act* out = nullptr; size_t op0 = 0, op1 = 0; };
    std::map<int, BlockInfo> blocks;
    Act* bottleneck(Act* x, int id, int inplanes, int planes, bool first, bool stride2) {
        blocks[id].in = x; blocks[id].op0 = ops.size();
        Act* r = bottleneck_body(x, id, inplanes, planes, first, stride2);
        blocks[id].out = r; blocks[id].op1 = ops.size();
        return r;
    }
    Act* bottleneck_body(Act* x, int id, int inplanes, int planes, bool first, bool stride2) {
        const std::string sid = std::to_string(id);
        const char st = "ABC"[id % 3];
        const int one[3] = {1, 1, 1};
        const int s2[3] = {1, 2, 2};
        const int* s = (first && stride2) ? s2 : one;
        const int kS[3] = {1, 3, 3}, kT[3] = {3, 1, 1};
        const std::string B = "block" + sid + "/";
        // variable creation order matters for BN auto-naming (SURVEY Appendix D)
        // BatchNorm fusion (ConvFuse): bn1, bnS, bnT and their ReLUs ride on the operand paths of the convs around them;
        // only bn3 (+ residual) keeps a pass of its own.  Every bn_apply below marked fused_site runs only with fusion off.
        Param* w1 = wd_weight("conv3_" + sid + "_1", {1, 1, 1, inplanes, planes});
        BN* bn1 = add_bn("", planes, false);
        const ConvGeo g1 = make_geo(x->D, x->H, x->W, one, s);
        const bool fz = (int64_t)x->N * g1.O[0] * g1.O[1] * g1.O[2] <= fuse_max_rows;      // this bottleneck is built fusable
        ConvFuse f1; if (fz) f1.out_bn = bn1;
        Act* y1 = conv(B + "conv1", x, w1, nullptr, one, s, planes, bn1, "", false, false, 0, &f1);
        Act* z1 = bn_apply(B + "bn1", 0, y1, bn1, nullptr, nullptr, nullptr, B + "conv1_bn_relu", false, /*fused_site=*/fz);
        const std::string nm = std::string("ST") + st + "_" + sid + "_2";
        Act* stout = nullptr;
        ConvFuse f3;                 // conv3's view of the ST output
        if (st == 'A') {          // p3d.py:56-63
            Param* wS = wd_weight(nm + "_S", {1, 3, 3, planes, planes});
            Param* bS = conv_weight(nm + "_S_bias", {planes});
            BN* bnS = add_bn("", planes, false);
            ConvFuse fS; fS.at = P3D_AT_RELU1; fS.src[0] = {y1, bn1, 1}; fS.ngate = 1; fS.gate[0] = {y1, bn1, 0}; fS.out_bn = bnS;
            if (!fz) fS = ConvFuse();
            Act* yS = conv(B + "convS", z1, wS, bS, kS, one, planes, bnS, "", false, false, 0, &fS);
            Act* zS = bn_apply(B + "bnS", 0, yS, bnS, nullptr, nullptr, nullptr, "", false, fz);
            Param* wT = wd_weight(nm + "_T", {3, 1, 1, planes, planes});
            Param* bT = conv_weight(nm + "_T_bias", {planes});
            BN* bnT = add_bn("", planes, false);
            ConvFuse fT; fT.at = P3D_AT_RELU1; fT.src[0] = {yS, bnS, 1}; fT.ngate = 1; fT.gate[0] = {yS, bnS, 0}; fT.out_bn = bnT;
            if (!fz) fT = ConvFuse();
            Act* yT = conv(B + "convT", zS, wT, bT, kT, one, planes, bnT, "", false, false, 0, &fT);
            stout = bn_apply(B + "bnT", 0, yT, bnT, nullptr, nullptr, nullptr, B + "st", false, fz);
            f3.at = P3D_AT_RELU1; f3.src[0] = {yT, bnT, 1}; f3.ngate = 1; f3.gate[0] = {yT, bnT, 0};
        } else if (st == 'B') {   // p3d.py:65-72
            Param* wS = wd_weight(nm + "_S", {1, 3, 3, planes, planes});
            Param* bS = conv_weight(nm + "_S_bias", {planes});
            BN* bnS = add_bn("", planes, false);
            // z1 feeds both siblings: convS (registered first, so last in backward) folds and publishes bn1 in the forward and,
            // in the backward, adds the raw gradient convT left in z1->g, gates it and reduces for bn1
            ConvFuse fS; fS.at = P3D_AT_RELU1; fS.src[0] = {y1, bn1, 1}; fS.ngate = 1; fS.gate[0] = {y1, bn1, 0}; fS.accum_in = true; fS.out_bn = bnS;
            if (!fz) fS = ConvFuse();
            Act* yS = conv(B + "convS", z1, wS, bS, kS, one, planes, bnS, "", false, false, /*sibling=*/1, &fS);
            Param* wT = wd_weight(nm + "_T", {3, 1, 1, planes, planes});
            Param* bT = conv_weight(nm + "_T_bias", {planes});
            BN* bnT = add_bn("", planes, false);
            ConvFuse fT; fT.at = P3D_AT_RELU1; fT.src[0] = {y1, bn1, 2}; fT.out_bn = bnT;
            if (!fz) fT = ConvFuse();
            Act* yT = conv(B + "convT", z1, wT, bT, kT, one, planes, bnT, "", false, false, /*sibling=*/2, &fT);
            stout = bn_apply(B + "bnST", 3, yS, bnS, yT, bnT, nullptr, B + "st", false, fz);
            f3.at = P3D_AT_RELU2; f3.src[0] = {yS, bnS, 1}; f3.src[1] = {yT, bnT, 1};
            f3.ngate = 2; f3.gate[0] = {yS, bnS, 0}; f3.gate[1] = {yT, bnT, 0};
        } else {                  // p3d.py:74-81
            Param* wS = wd_weight(nm + "_S", {1, 3, 3, planes, planes});
            Param* bS = conv_weight(nm + "_S_bias", {planes});
            BN* bnS = add_bn("", planes, false);
            ConvFuse fS; fS.at = P3D_AT_RELU1; fS.src[0] = {y1, bn1, 1}; fS.ngate = 1; fS.gate[0] = {y1, bn1, 0}; fS.out_bn = bnS;
            if (!fz) fS = ConvFuse();
            Act* yS = conv(B + "convS", z1, wS, bS, kS, one, planes, bnS, "", false, false, 0, &fS);
            Act* zS = bn_apply(B + "bnS", 0, yS, bnS, nullptr, nullptr, nullptr, "", false, fz);
            Param* wT = wd_weight(nm + "_T", {3, 1, 1, planes, planes});
            Param* bT = conv_weight(nm + "_T_bias", {planes});
            BN* bnT = add_bn("", planes, false);
            // zS also reaches conv3 through the skip: conv3's input gradient leaves its raw result in zS->g, convT's adds its
            // own, gates and reduces for bnS
            ConvFuse fT; fT.at = P3D_AT_RELU1; fT.src[0] = {yS, bnS, 1}; fT.ngate = 1; fT.gate[0] = {yS, bnS, 0}; fT.accum_in = true; fT.out_bn = bnT;
            if (!fz) fT = ConvFuse();
            Act* yT = conv(B + "convT", zS, wT, bT, kT, one, planes, bnT, "", false, false, 0, &fT);
            stout = bn_apply(B + "bnT", 4, yT, bnT, zS, nullptr, nullptr, B + "st", false, fz);
            f3.at = P3D_AT_RELU2; f3.src[0] = {yS, bnS, 0}; f3.src[1] = {yT, bnT, 1};
            f3.ngate = 1; f3.gate[0] = {yT, bnT, 0}; f3.raw = zS; f3.raw_flag = zS->last_flag;      // the flag of bnT's skip read
        }
        if (!fz) f3 = ConvFuse();
        Param* w3 = wd_weight("conv3_" + sid + "_3", {1, 1, 1, planes, planes * 4});
        BN* bn3 = add_bn("", planes * 4, false);
        Act* y3 = conv(B + "conv3", stout, w3, nullptr, one, one, planes * 4, bn3, "", false, false, 0, &f3);
        if (first) {              // p3d.py:124-127
            Param* wp = wd_weight("dw3d_" + sid, {1, 1, 1, inplanes, planes * 4});
            BN* bnp = add_bn("", planes * 4, false);
            Act* yp = conv(B + "proj", x, wp, nullptr, one, s, planes * 4, bnp, "");
            return bn_apply(B + "bn3", 2, y3, bn3, yp, bnp, nullptr, B + "out");
        }
        return bn_apply(B + "bn3", 1, y3, bn3, x, nullptr, nullptr, B + "out");
    }

    // p3d.py:170-195: stem + three stages + temporal pools, shared verbatim by every head.  skip[0..1] are
    // where pool2 / pool3 land (channel slices of decoder concat buffers for the unet head, or null).
    Act* stem_out = nullptr;     // conv1_custom_bn_relu, which the unet++ head pools a second time (p3d.py:408)
    void build_encoder(Act* skip2, Act* skip3, Act*& pool2, Act*& pool3, Act*& pool4) {
        const int B = cfg.batch, T = cfg.frames, H = cfg.height, W = cfg.width, b = cfg.base;
        if (T % 16 || H % 16 || W % 16) throw P3dError("frames/height/width must be multiples of 16");
        if (b % 8) throw P3dError("base must be a multiple of 8");
        x_in = new_act("x", B, T, H, W, 3, /*with_grad=*/false);
        // p3d.py:172-177
        const int k177[3] = {1, 7, 7}, s122[3] = {1, 2, 2};
        Param* w0 = wd_weight("firstconv1", {1, 7, 7, 3, b});
        BN* bn0 = add_bn("", b, true);
        Act* c1 = conv("stem/conv", x_in, w0, nullptr, k177, s122, b, bn0, "conv1_custom", /*stem=*/true);
        Act* a1 = bn_apply("stem/bn", 0, c1, bn0, nullptr, nullptr, nullptr, "conv1_custom_bn_relu");
        stem_out = a1;
        const int k233[3] = {2, 3, 3}, s222[3] = {2, 2, 2}, k211[3] = {2, 1, 1}, s211[3] = {2, 1, 1};
        Act* cur = maxpool("pool1", a1, k233, s222, nullptr, "pool1");
        int id = 0, inpl = b;
        const int planes[3] = {b, 2 * b, 4 * b};
        Act* skips[3] = {skip2, skip3, nullptr};
        Act* outs[3] = {nullptr, nullptr, nullptr};
        const char* pool_names[3] = {"pool2", "pool3", "pool4"};
        for (int stage = 0; stage < 3; ++stage) {
            for (int j = 0; j < cfg.blocks[stage]; ++j) {
                cur = bottleneck(cur, id, inpl, planes[stage], j == 0, stage > 0);
                inpl = planes[stage] * 4;
                ++id;
            }
            cur = maxpool(pool_names[stage], cur, k211, s211, skips[stage], pool_names[stage]);
            outs[stage] = cur;
        }
        pool2 = outs[0]; pool3 = outs[1]; pool4 = outs[2];
    }

    void build_unet() {
        const int B = cfg.batch, T = cfg.frames, H = cfg.height, W = cfg.width, b = cfg.base;
        const int k233[3] = {2, 3, 3}, s222[3] = {2, 2, 2};
        // concat buffers of the decoder (p3d.py:203,208): [deconvN_re | poolM]
        Act* cat1 = new_act("deconv1_concat", B, T / 8, H / 8, W / 8, 16 * b);
        Act* cat2 = new_act("deconv2_concat", B, T / 4, H / 4, W / 4, 8 * b);
        Act *pool2, *pool3, *pool4;
        build_encoder(new_view(cat2, 4 * b, 4 * b, "pool2"), new_view(cat1, 8 * b, 8 * b, "pool3"), pool2, pool3, pool4);
        // decoder p3d.py:200-219
        const int k133[3] = {1, 3, 3}, k333[3] = {3, 3, 3}, k111[3] = {1, 1, 1}, s111[3] = {1, 1, 1};
        {
            Param* k = conv_weight("conv3d_transpose/kernel", {1, 3, 3, 8 * b, 16 * b});
            Param* bi = add_param("conv3d_transpose/bias", {8 * b}, true, INIT_ZEROS);
            BN* bn = add_bn("deconv1_bn", 8 * b, true);
            Act* y = deconv("deconv1", pool4, k, bi, k133, s222, 8 * b, bn, "");
            bn_apply("deconv1_bn", 0, y, bn, nullptr, nullptr, new_view(cat1, 0, 8 * b, "deconv1_re"), "");
        }
        {
            Param* k = conv_weight("conv3d_transpose_1/kernel", {2, 3, 3, 4 * b, 16 * b});
            Param* bi = add_param("conv3d_transpose_1/bias", {4 * b}, true, INIT_ZEROS);
            BN* bn = add_bn("deconv2_bn", 4 * b, true);
            Act* y = deconv("deconv2", cat1, k, bi, k233, s222, 4 * b, bn, "");
            bn_apply("deconv2_bn", 0, y, bn, nullptr, nullptr, new_view(cat2, 0, 4 * b, "deconv2_re"), "");
        }
        Act* d3;
        {
            Param* k = conv_weight("conv3d_transpose_2/kernel", {3, 3, 3, 2 * b, 8 * b});
            Param* bi = add_param("conv3d_transpose_2/bias", {2 * b}, true, INIT_ZEROS);
            BN* bn = add_bn("deconv3_bn", 2 * b, true);
            Act* y = deconv("deconv3", cat2, k, bi, k333, s222, 2 * b, bn, "", /*bn_has_dropout=*/true);
            d3 = bn_apply("deconv3_bn", 0, y, bn, nullptr, nullptr, nullptr, "deconv3_re", /*dropout=*/true);
        }
        Param* k4 = conv_weight("conv3d/kernel", {1, 1, 1, 2 * b, b / 2});
        Param* b4 = add_param("conv3d/bias", {b / 2}, true, INIT_ZEROS);
        Act* c4 = conv("deconv4_conv1", d3, k4, b4, k111, s111, b / 2, nullptr, "deconv4_conv1");
        Param* k5 = conv_weight("conv3d_transpose_3/kernel", {3, 3, 3, 1, b / 2});
        Param* b5 = add_param("conv3d_transpose_3/bias", {1}, true, INIT_ZEROS);
        head(c4, k5, b5);
    }

    // p3d_concat (p3d.py:224-276, --structure concat): three skip deconvs to 4x28x28, channel concat, one dense
    // 3x3x3 conv, one deconv, and a 1-channel deconv WITHOUT sigmoid.
    void build_concat() {
        const int B = cfg.batch, T = cfg.frames, H = cfg.height, W = cfg.width, b = cfg.base;
        const int k333[3] = {3, 3, 3}, s111[3] = {1, 1, 1}, s222[3] = {2, 2, 2}, s444[3] = {4, 4, 4};
        Act *pool2, *pool3, *pool4;
        build_encoder(nullptr, nullptr, pool2, pool3, pool4);
        Act* cat = new_act("concatenator", B, T / 4, H / 4, W / 4, 14 * b);
        auto up = [&](const char* name, const char* bn_name, Act* x, int filters, const int* s, int coff) {
            Param* k = conv_weight(std::string(name) + "/kernel", {3, 3, 3, filters, x->C});
            Param* bi = add_param(std::string(name) + "/bias", {filters}, true, INIT_ZEROS);
            BN* bn = add_bn(bn_name, filters, true);
            Act* y = deconv(name, x, k, bi, k333, s, filters, bn, "");
            bn_apply(bn_name, 0, y, bn, nullptr, nullptr, new_view(cat, coff, filters, ""), "");
        };
        up("deconv_pool2", "deconv_pool2_bn", pool2, 2 * b, s111, 0);
        up("deconv_pool3", "deconv_pool3_bn", pool3, 4 * b, s222, 2 * b);
        up("deconv_pool4", "deconv_pool4_bn", pool4, 8 * b, s444, 6 * b);
        Param* kc = conv_weight("conv_concat/kernel", {3, 3, 3, 14 * b, 8 * b});
        Param* bc = add_param("conv_concat/bias", {8 * b}, true, INIT_ZEROS);
        BN* bnc = add_bn("conv_concat_bn", 8 * b, true);
        Act* yc = conv("conv_concat", cat, kc, bc, k333, s111, 8 * b, bnc, "");
        Act* zc = bn_apply("conv_concat_bn", 0, yc, bnc, nullptr, nullptr, nullptr, "conv_concat");
        Param* kr = conv_weight("deconv_revise/kernel", {3, 3, 3, 2 * b, 8 * b});
        Param* br = add_param("deconv_revise/bias", {2 * b}, true, INIT_ZEROS);
        BN* bnr = add_bn("deconv1_revise_bn", 2 * b, true);
        Act* yr = deconv("deconv_revise", zc, kr, br, k333, s222, 2 * b, bnr, "", /*bn_has_dropout=*/true);
        Act* zr = bn_apply("deconv1_revise_bn", 0, yr, bnr, nullptr, nullptr, nullptr, "deconv1_revise", /*dropout=*/true);
        Param* kp = conv_weight("predict_revise/kernel", {3, 3, 3, 1, 2 * b});
        Param* bp = add_param("predict_revise/bias", {1}, true, INIT_ZEROS);
        head(zr, kp, bp, /*with_sigmoid=*/false);
    }

    // ---- self attention, utils/network.py:157-192 (mode 'bn', sub_size 2) --------------------------------------
    struct AttnParams { Param *wf, *bf, *wg, *bg, *wh, *bh, *wo, *bo, *gamma; BN* bn; int ch; std::string name; };
    // p3d_set_attention_mode: 0 = per site (flash where the score matrix of the site has at least attn_flash_min_scores elements),
    // 1 = GEMMs around stored scores everywhere, 2 = flash wherever the kernels exist (ch in 32..256)
    int attn_mode = 0;
    int64_t attn_flash_min_scores = (int64_t)1 << 24;         // 64 MiB of scores per buffer (measured crossover: DESIGN.md)
    std::vector<std::function<void()>> attn_gemm_alloc;
    // variables in the reference's creation order: name/conv3d{,_1,_2}, an unnamed top-level conv3d, an unnamed
    // batch_normalization, then the top-level scalar 'gamma'+name (initialised to 0)
    AttnParams attn_declare(const std::string& name, int ch) {
        AttnParams a;
        a.name = name; a.ch = ch;
        const int ci = std::max(1, ch / 8);
        if (ci % 4) throw P3dError("attention needs channel counts that are multiples of 32 (base multiple of 16)");
        a.wf = conv_weight(name + "/conv3d/kernel", {1, 1, 1, ch, ci});   a.bf = add_param(name + "/conv3d/bias", {ci}, true, INIT_ZEROS);
        a.wg = conv_weight(name + "/conv3d_1/kernel", {1, 1, 1, ch, ci}); a.bg = add_param(name + "/conv3d_1/bias", {ci}, true, INIT_ZEROS);
        a.wh = conv_weight(name + "/conv3d_2/kernel", {1, 1, 1, ch, ch}); a.bh = add_param(name + "/conv3d_2/bias", {ch}, true, INIT_ZEROS);
        const std::string oc = unique("conv3d");
        a.wo = conv_weight(oc + "/kernel", {1, 1, 1, ch, ch}); a.bo = add_param(oc + "/bias", {ch}, true, INIT_ZEROS);
        a.bn = add_bn("", ch, true);
        a.gamma = add_param("gamma" + name, {1}, true, INIT_ZEROS);
        return a;
    }
    // x -> relu(bn(conv(softmax(g f^T) h))) * gamma + x; with subsample the keys f and values h are max-pooled by 2
    // (utils/network.py:178-181; the query pool has size sub_size/2 = 1).  `dropout` folds the tf.layers.dropout
    // that follows the last block (p3d.py:388) into the mixing pass.
    Act* attn_run(const AttnParams& ap, Act* x, bool subsample, const std::string& out_name, bool dropout = false) {
        const int one[3] = {1, 1, 1}, two[3] = {2, 2, 2};
        const int ch = ap.ch, ci = ch / 8, B = x->N;
        if (x->C != ch) throw P3dError("attention declared for another channel count");
        const std::string& nm = ap.name;
        Act* f = conv(nm + "/f", x, ap.wf, ap.bf, one, one, ci, nullptr, "");
        Act* gq = conv(nm + "/g", x, ap.wg, ap.bg, one, one, ci, nullptr, "");
        Act* h = conv(nm + "/h", x, ap.wh, ap.bh, one, one, ch, nullptr, "");
        if (subsample) {
            if ((x->D | x->H | x->W) & 1) throw P3dError("attention sub-sampling needs even extents ('valid' pooling)");
            f = maxpool(nm + "/pool_f", f, two, two, nullptr, "");
            h = maxpool(nm + "/pool_h", h, two, two, nullptr, "");
        }
        const int Ng = gq->D * gq->H * gq->W, Nf = f->D * f->H * f->W, Nfp = (Nf + 3) / 4 * 4;
        const bool pad = Nfp != Nf;
        Act* o = new_act(nm + "/o", B, x->D, x->H, x->W, ch);
        // Two executions of the core (p3d_set_attention_mode): score tiles recomputed on chip (attention_flash.hip: lse + row
        // dots are all it keeps), or three GEMMs per direction around a stored score matrix.  The GEMM path's buffers
        // (2 x B*Ng*Nf floats) are only allocated for sites that may take it.
        const bool can_flash = p3d_flash_attn_ok(ch);
        const bool auto_flash = can_flash && (int64_t)B * Ng * Nfp >= attn_flash_min_scores;
        float* lse = can_flash ? dalloc<float>((int64_t)B * Ng) : nullptr;
        float* dsum = can_flash ? dalloc<float>((int64_t)B * Ng) : nullptr;
        struct GemmBufs { float *sbuf = nullptr, *dsbuf = nullptr, *fpad = nullptr, *hpad = nullptr, *dfpad = nullptr, *dhpad = nullptr; };
        GemmBufs* gb = new GemmBufs();           // lives as long as the handle (ops capture it)
        auto ensure_gemm = [=]() {
            if (gb->sbuf) return;
            gb->sbuf = dalloc<float>((int64_t)B * Ng * Nfp);       // scores, then the attention map beta (kept for backward)
            gb->dsbuf = dalloc<float>((int64_t)B * Ng * Nfp);      // d beta, then d scores
            if (pad) {
                gb->fpad = dalloc<float>((int64_t)B * Nfp * ci); gb->hpad = dalloc<float>((int64_t)B * Nfp * ch);
                gb->dfpad = dalloc<float>((int64_t)B * Nfp * ci); gb->dhpad = dalloc<float>((int64_t)B * Nfp * ch);
            }
        };
        if (!auto_flash) ensure_gemm();
        attn_gemm_alloc.push_back(ensure_gemm);
        bool* ran_flash = new bool(false);       // what the last forward of this site ran (its backward follows)
        auto flash_args = [=]() {
            FlashAttnArgs a;
            memset(&a, 0, sizeof(a));
            a.B = B; a.Ng = Ng; a.Nf = Nf; a.ch = ch;
            a.g = gq->p; a.ldg = gq->ld; a.f = f->p; a.ldf = f->ld; a.h = h->p; a.ldh = h->ld;
            a.o = o->p; a.ldo = o->ld; a.lse = lse;
            a.d_o = o->g; a.lddo = o->ld; a.dsum = dsum;
            a.dg = gq->g; a.lddg = gq->ld; a.df = f->g; a.lddf = f->ld; a.dh = h->g; a.lddh = h->ld;
            return a;
        };
        char* flg = consume(gq); char* flf = consume(f); char* flh = consume(h);
        {
            Op op;
            op.name = nm + "/core"; op.kind = "attention";
            op.flops = 2.0 * B * (double)Ng * Nf * (ci + ch);
            op.bytes = 4.0 * B * ((double)Ng * Nfp * 4 + (double)Ng * (ci + ch) + (double)Nf * (ci + ch));
            op.bflops = 2 * op.flops; op.bbytes = 2 * op.bytes;
            // the stored-score execution on this site's tensors, as they stand when the op runs (AttnCore, net.hip)
            auto core = [=]() {
                AttnCore a;
                a.B = B; a.Ng = Ng; a.Nf = Nf; a.ch = ch; a.gD = gq->D; a.gH = gq->H; a.gW = gq->W;
                a.g = gq->p; a.ldg = gq->ld; a.f = f->p; a.h = h->p; a.o = o->p; a.ldo = o->ld;
                a.d_o = o->g; a.dg = gq->g; a.df = f->g; a.dh = h->g;
                a.sbuf = gb->sbuf; a.dsbuf = gb->dsbuf; a.fpad = gb->fpad; a.hpad = gb->hpad; a.dfpad = gb->dfpad; a.dhpad = gb->dhpad;
                return a;
            };
            const double pair_flops = 2.0 * B * (double)Ng * Nf * (ci + ch);
            const double operand_bytes = 4.0 * B * ((double)Ng * (ci + ch) + (double)Nf * (ci + ch));
            op.fwd = [=](const Ctx& c) {
                *ran_flash = can_flash && (attn_mode == 2 || (attn_mode == 0 && auto_flash));
                if (*ran_flash) {
                    launch(c, "flash_fwd_kernel", pair_flops, operand_bytes, [&]() { return p3d_flash_attn_fwd(flash_args(), c.s); });
                    return;
                }
                if (!gb->sbuf) throw P3dError("attention GEMM path without its score buffers (p3d_set_attention_mode allocates them)");
                core().forward(c);
            };
            op.bwd = [=](const Ctx& c) {
                if (*flg || *flf || *flh) throw P3dError("attention operands have one consumer each");
                if (*ran_flash) {
                    if (c.dry) return;
                    const FlashAttnArgs a = flash_args();
                    // one entry point, three launches (row dots; dg per query tile; df, dh per key tile)
                    launch(c, "flash_bwd(rowdot + q + k kernels)", 3.2 * pair_flops, 3 * operand_bytes, [&]() { return p3d_flash_attn_bwd(a, c.s); });
                    return;
                }
                core().backward(c);
            };
            ops.push_back(op);
        }
        Act* y = conv(nm + "/out", o, ap.wo, ap.bo, one, one, ch, ap.bn, "");
        Act* r = bn_apply(nm + "/out_bn", 0, y, ap.bn, nullptr, nullptr, nullptr, "");
        Act* z = new_act(out_name, B, x->D, x->H, x->W, ch);
        char* flr = consume(r); char* flx = consume(x);
        {
            Op op;
            op.name = nm + "/mix"; op.kind = "attention_mix";
            op.bytes = 4.0 * 3 * x->rows() * ch; op.bbytes = 4.0 * 5 * x->rows() * ch;
            op.owns = {ap.gamma};
            Param* gamma = ap.gamma;
            auto mk = [=](const Ctx& c) { return attn_mix_args(x->rows(), ch, r->p, r->ld, x->p, x->ld, gamma->p, z->p, z->ld, z->g, r->g, x->g, *flx, gamma->g, c, dropout); };
            op.fwd = [=](const Ctx& c) { attn_mix_forward(c, mk(c)); };
            op.bwd = [=](const Ctx& c) {
                if (*flr) throw P3dError("attention branch has one consumer");
                attn_mix_backward(c, mk(c));
            };
            ops.push_back(op);
        }
        return z;
    }

    // p3d_unetplusplus_nonsa (p3d.py:401-459): the nested UNet++ head without the attention blocks.  Every layer
    // is utils/network.py:100-110: named tf.layers.conv3d / conv3d_transpose + an UNNAMED batch_normalization
    // (it follows `training` and continues the backbone's counter in the reference's call order) + ReLU.
    // Variables are therefore created in the reference's order, but the ops run in an order in which each
    // concat buffer's whole consumer (the x_i_j conv) comes after every consumer of one of its slices -- see
    // consume().  Concats are zero-copy: producers write channel slices of the buffers below.
    // with sa = true: p3d_unetplusplus_ds (p3d.py:340-397), the same head with attention() on x_4_0, x_3_1, x_2_2
    // and (keys / values pooled by 2, followed by the dropout) x_1_3
    void build_unetpp(bool sa) {
        const int B = cfg.batch, T = cfg.frames, H = cfg.height, W = cfg.width, b = cfg.base;
        const int s111[3] = {1, 1, 1}, s222[3] = {2, 2, 2}, k211[3] = {2, 1, 1}, s211[3] = {2, 1, 1};
        Act* cat31 = new_act("cat_x_3_1", B, T / 8, H / 8, W / 8, 16 * b);    // [x_3_0 | upx_4_0]
        Act* cat21 = new_act("cat_x_2_1", B, T / 4, H / 4, W / 4, 8 * b);     // [x_2_0 | upx_3_0]
        Act* cat22 = new_act("cat_x_2_2", B, T / 4, H / 4, W / 4, 8 * b);     // [x_2_1 | upx_3_1]
        Act* cat11 = new_act("cat_x_1_1", B, T / 2, H / 2, W / 2, 3 * b);     // [x_1_0 | upx_2_0]
        Act* cat12 = new_act("cat_x_1_2", B, T / 2, H / 2, W / 2, 4 * b);     // [x_1_1 | upx_2_1]
        Act* cat13 = new_act("cat_x_1_3", B, T / 2, H / 2, W / 2, 4 * b);     // [x_1_2 | upx_2_2]
        Act *x_2_0, *x_3_0, *x_4_0;
        build_encoder(new_view(cat21, 0, 4 * b, "pool2"), new_view(cat31, 0, 8 * b, "pool3"), x_2_0, x_3_0, x_4_0);
        Act* x_1_0 = maxpool("x_1_0", stem_out, k211, s211, new_view(cat11, 0, b, ""), "x_1_0");
        (void)x_1_0;
        struct Layer { Param *k, *bias; BN* bn; int filters; int kk[3]; bool up; };
        std::map<std::string, Layer> L;
        auto declare = [&](const char* name, bool up, int cin, int filters, int kd) {
            Layer l;
            l.up = up; l.filters = filters; l.kk[0] = kd; l.kk[1] = 3; l.kk[2] = 3;
            l.k = up ? conv_weight(std::string(name) + "/kernel", {kd, 3, 3, filters, cin})
                     : conv_weight(std::string(name) + "/kernel", {kd, 3, 3, cin, filters});
            l.bias = add_param(std::string(name) + "/bias", {filters}, true, INIT_ZEROS);
            l.bn = add_bn("", filters, true);
            L[name] = l;
        };
        // reference creation order (p3d.py:371-387 / 435-451)
        AttnParams sa40, sa31, sa22, sa13;
        if (sa) sa40 = attn_declare("x_4_0_sa", 16 * b);
        declare("upx_4_0", true, 16 * b, 8 * b, 1);
        declare("x_3_1", false, 16 * b, 8 * b, 2);
        if (sa) sa31 = attn_declare("x_3_1_sa", 8 * b);
        declare("upx_3_0", true, 8 * b, 4 * b, 2);
        declare("x_2_1", false, 8 * b, 4 * b, 3);
        declare("upx_3_1", true, 8 * b, 4 * b, 2);
        declare("x_2_2", false, 8 * b, 4 * b, 3);
        if (sa) sa22 = attn_declare("x_2_2_sa", 4 * b);
        declare("upx_2_0", true, 4 * b, 2 * b, 3);
        declare("x_1_1", false, 3 * b, 2 * b, 3);
        declare("upx_2_1", true, 4 * b, 2 * b, 3);
        declare("x_1_2", false, 4 * b, 2 * b, 3);
        declare("upx_2_2", true, 4 * b, 2 * b, 3);
        declare("x_1_3", false, 4 * b, 2 * b, 3);
        if (sa) sa13 = attn_declare("x_1_3_sa", 2 * b);
        auto run = [&](const char* name, Act* x, Act* out, bool dropout = false) -> Act* {
            const Layer& l = L.at(name);
            Act* y = l.up ? deconv(name, x, l.k, l.bias, l.kk, s222, l.filters, l.bn, "", dropout)
                          : conv(name, x, l.k, l.bias, l.kk, s111, l.filters, l.bn, "", false, dropout);
            return bn_apply(std::string(name) + "_bn", 0, y, l.bn, nullptr, nullptr, out, name, dropout);
        };
        if (sa) x_4_0 = attn_run(sa40, x_4_0, false, "x_4_0_sa");
        run("upx_4_0", x_4_0, new_view(cat31, 8 * b, 8 * b, ""));
        run("upx_3_0", x_3_0, new_view(cat21, 4 * b, 4 * b, ""));
        run("upx_2_0", x_2_0, new_view(cat11, b, 2 * b, ""));
        Act* x_3_1 = run("x_3_1", cat31, nullptr);
        if (sa) x_3_1 = attn_run(sa31, x_3_1, false, "x_3_1_sa");
        Act* x_2_1 = run("x_2_1", cat21, new_view(cat22, 0, 4 * b, ""));
        run("x_1_1", cat11, new_view(cat12, 0, 2 * b, ""));
        run("upx_3_1", x_3_1, new_view(cat22, 4 * b, 4 * b, ""));
        run("upx_2_1", x_2_1, new_view(cat12, 2 * b, 2 * b, ""));
        Act* x_2_2 = run("x_2_2", cat22, nullptr);
        if (sa) x_2_2 = attn_run(sa22, x_2_2, false, "x_2_2_sa");
        run("x_1_2", cat12, new_view(cat13, 0, 2 * b, ""));
        run("upx_2_2", x_2_2, new_view(cat13, 2 * b, 2 * b, ""));
        Act* x_1_3 = run("x_1_3", cat13, nullptr, /*dropout=*/!sa);
        if (sa) x_1_3 = attn_run(sa13, x_1_3, true, "x_1_3_sa", /*dropout=*/true);
        Param* kh = conv_weight("x_0_1/kernel", {3, 3, 3, 1, 2 * b});
        Param* bh = add_param("x_0_1/bias", {1}, true, INIT_ZEROS);
        head(x_1_3, kh, bh);
    }

    // results = sigmoid(conv3d_transpose(x, 1, 3, 2)) (p3d.py:217-219) + Smooth-L1 (train.py:156-159)
    bool head_sigmoid = true;
    // transpose = false: the stride-1 tf.layers.conv3d(x, 1, 3, 1, 'same') of gn/p3d_gn.py:537 instead
    void head(Act* x, Param* k, Param* bias, bool with_sigmoid = true, bool transpose = true) {
        head_sigmoid = with_sigmoid;
        // the head's kernels address x as dense [rows][C] (HeadArgs has no row stride)
        if (x->ld != x->C) throw P3dError("head input " + x->name + " has a row stride of " + std::to_string(x->ld) + ", not its " +
                                          std::to_string(x->C) + " channels");
        const int up = transpose ? 2 : 1;
        logits = new_act("logits", x->N, up * x->D, up * x->H, up * x->W, 1, false);
        pred = new_act("pred", x->N, up * x->D, up * x->H, up * x->W, 1, false);
        d_dlogits = dalloc<float>(pred->rows());
        d_y = dalloc<float>(pred->rows());
        d_loss = dalloc<double>(1);
        {   // the per-map loss's scratch, sized from the B*T maps of H*W: a step allocates nothing (captured steps stay valid)
            size_t md = 0, mc = 0;
            p3d_map_loss_scratch((long long)pred->N * pred->D, (long long)pred->H * pred->W, &md, &mc);
            d_map_scratch = dalloc<double>((int64_t)md);
            d_map_cnt = dalloc<unsigned>((int64_t)mc);
            HIPCHECK(fill_now(d_map_cnt, 0, mc * sizeof(unsigned), stream));
        }
        char* xflag = consume(x);
        Op op;
        op.name = "results"; op.kind = transpose ? "head_deconv" : "head_conv";
        op.flops = 2.0 * x->rows() * 27 * x->C;
        op.bytes = 4.0 * (x->rows() * (double)x->C + 2.0 * pred->rows());
        op.bflops = 2 * op.flops; op.bbytes = 4.0 * (3.0 * x->rows() * (double)x->C + 2.0 * pred->rows());
        op.owns = {k, bias};
        auto mk = [=]() { return head_args(x->p, x->N, x->D, x->H, x->W, x->C, k->p, bias->p, logits->p, pred->p, with_sigmoid, d_dlogits, x->g, k->g, bias->g); };
        hipEvent_t head_fork = new_fork_event();
        op.fwd = [=](const Ctx& c) { head_forward(c, mk(), transpose); };
        op.bwd = [=](const Ctx& c) {
            if (*xflag) throw P3dError("head input gradient must be the first writer");
            // the filter gradient is a weight gradient like any other: side stream, off the critical path
            on_side_stream(c, head_fork, [=](const Ctx& sc) { head_filter_gradient(sc, mk(), transpose); });
            head_input_gradient(c, mk(), transpose);
        };
        ops.push_back(op);
    }
