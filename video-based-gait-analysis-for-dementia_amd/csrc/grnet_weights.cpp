// The weight loader: reference state_dict keys -> BatchNorm-folded weights in the layouts the kernels read, and the entry points that feed it.
#include "grnet_impl.h"

namespace {
constexpr double kBnEps = 1e-5;   // nn.BatchNorm2d default eps
}

// ------------------------------------------------------------------ weights
const HostTensor* grnet::find(const std::string& k) const {
    auto it = tensors.find(k);
    return it == tensors.end() ? nullptr : &it->second;
}

int grnet::upload(const std::vector<float>& h, float** d) {
    int rc = dev_alloc(d, h.size());
    if (rc) return rc;
    if (hipMemcpy(*d, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        return fail(GRNET_EHIP, "hipMemcpy H2D failed");
    return 0;
}

// Fold BN (fp64) and pack to [tap][CinPad][CoutPad].
int grnet::pack_conv(ConvLayer& L) {
    const int cin = L.cin_w, ks = L.ks, taps = ks * ks;
    const int TC = conv_pick_tc(L.cout);
    const bool bf = dtype == 1;                            // bf16: [CinPad/32][tap][CoutPad][32]: a chunk's rows are contiguous for LDS-DMA
    L.cin_pad = bf ? (L.in.c + L.in2.c + 31) / 32 * 32 : (cin + kConvCK - 1) / kConvCK * kConvCK;
    if (L.in2.c && (!bf || ks != 1 || L.in.c % 32 != 0 || L.segs.size() != 1 || L.seg2.cout != L.cout)) return fail(GRNET_ESTATE, "a two-input launch is a bf16 1x1 convolution with one weight segment per input");
    L.cout_pad = bf ? (L.cout + 31) / 32 * 32 : (L.cout + TC - 1) / TC * TC;
    std::vector<float> wp((size_t)taps * L.cin_pad * L.cout_pad, 0.f), bp(L.cout_pad, 0.f);
    // Every eligible 3x3 stride-1 layer takes a Winograd F(4x4,3x3) kernel: on 56x56 maps layer1, upsample heads, PARE head, transition1's
    // 256 -> 32 and the 32 -> 32 convolutions of the HR branch; on 28x28 maps the upsample-head layers and the 64 -> 64 convolutions of
    // the HR branch (conv_wino4.hip); on 14x14 / 7x7 maps the 128- / 256-channel HR branches and the 256 -> 256 upsample-head layer
    // (conv_wino4s.hip).  GRNET_WINO4=0 leaves every layer on the direct kernels (as GRNET_OPT_WINOGRAD = 0 does at run time).
    static const int wino4_env = GRNET_AB(WINO4, 2);
    const bool wino4 = !bf && wino4_env && conv_wino4_eligible(L.in.c, L.cout, L.ks, L.stride, L.in.h, L.in.w, (int)L.adds.size()) && L.cin_pad % 8 == 0 &&
                       L.cout_pad % (L.cout % 64 == 0 ? 64 : 32) == 0 && (L.adds.empty() || L.adds[0].shift == 0) &&
                       (L.in.w == 56 || (L.in.c >= 64 && L.cout % 64 == 0));
    const bool wino4s = !bf && wino4_env && cin == L.in.c && conv_wino4s_eligible(L.in.c, L.cout, L.ks, L.stride, L.in.h, L.in.w, (int)L.adds.size()) &&
                        (L.adds.empty() || L.adds[0].shift == 0);          // the small maps: conv_wino4s.hip
    static const int stem_env = GRNET_AB(STEM, 1);
    const bool stem_shape = cin == L.in.c && L.segs.size() == 1 && conv_stem_eligible(L.in.c, L.cout, L.ks, L.stride, L.in.h, L.in.w, (int)L.adds.size());
    // GRNET_STEM is the fp32 A/B switch only: a bf16 plan built for conv_bf16_stem (GRNET_BF16_STEM) has no NHWC copy of the frames, so its first
    // convolution MUST get the stem kernel's weights whatever GRNET_STEM says (round-4 advice: the generic kernel then read fp32 NCHW frames as NHWC bf16)
    const bool stem = !bf && stem_env && stem_shape, stem_bf = bf && bf16_stem && stem_shape;
    if (bf && bf16_stem && L.in.slot == View::kFrames && !stem_bf)
        return fail(GRNET_ESTATE, "bf16 plan without a conversion launch, but its first convolution is not eligible for conv_bf16_stem");
    std::vector<double> wfold(wino4 || wino4s || stem || stem_bf ? (size_t)L.cout * cin * 9 : 0);     // BN-folded weights (cout, cin, 3, 3) for the filter transform
    int co0 = 0;
    for (auto& s : L.segs) {
        const HostTensor* w = find(s.wkey);
        if (!w) return fail(GRNET_ENOENT, "missing tensor " + s.wkey);
        if (w->shape.size() != 4 || w->shape[0] != s.cout || w->shape[1] != cin || w->shape[2] != ks || w->shape[3] != ks)
            return fail(GRNET_EINVAL, "bad shape for " + s.wkey);
        std::vector<double> scale(s.cout, 1.0), shift(s.cout, 0.0);
        if (!s.biaskey.empty()) {
            const HostTensor* bt = find(s.biaskey);
            if (!bt || (int)bt->numel() != s.cout) return fail(GRNET_ENOENT, "missing tensor " + s.biaskey);
            for (int c = 0; c < s.cout; ++c) shift[c] = bt->data[c];
        }
        if (!s.bnprefix.empty()) {
            const HostTensor *g = find(s.bnprefix + ".weight"), *be = find(s.bnprefix + ".bias"),
                             *m = find(s.bnprefix + ".running_mean"), *v = find(s.bnprefix + ".running_var");
            if (!g || !be || !m || !v) return fail(GRNET_ENOENT, "missing BatchNorm tensors " + s.bnprefix + ".*");
            if ((int)g->numel() != s.cout) return fail(GRNET_EINVAL, "bad BatchNorm size " + s.bnprefix);
            for (int c = 0; c < s.cout; ++c) {
                const double sc = (double)g->data[c] / std::sqrt((double)v->data[c] + kBnEps);
                shift[c] = (double)be->data[c] + (shift[c] - (double)m->data[c]) * sc;
                scale[c] = sc;
            }
        }
        for (int co = 0; co < s.cout; ++co) {
            bp[co0 + co] = (float)shift[co];
            for (int ci = 0; ci < cin; ++ci)
                for (int t = 0; t < taps; ++t) {
                    const double wv = (double)w->data[((size_t)co * cin + ci) * taps + t] * scale[co];
                    wp[bf ? ((((size_t)(ci / 32) * taps + t) * L.cout_pad + co0 + co) * 32 + ci % 32) : ((size_t)t * L.cin_pad + ci) * L.cout_pad + co0 + co] = (float)wv;
                    if (wino4 || wino4s || stem || stem_bf) wfold[((size_t)(co0 + co) * cin + ci) * 9 + t] = wv;
                }
        }
        co0 += s.cout;
    }
    if (L.in2.c) {                                         // the second input's 1x1 weights behind the first's input channels, its BatchNorm shift added to the bias
        const ConvSeg& s2 = L.seg2;
        const int cin2 = L.in2.c;
        const HostTensor* w = find(s2.wkey);
        if (!w) return fail(GRNET_ENOENT, "missing tensor " + s2.wkey);
        if (w->shape.size() != 4 || w->shape[0] != s2.cout || w->shape[1] != cin2 || w->shape[2] != 1 || w->shape[3] != 1) return fail(GRNET_EINVAL, "bad shape for " + s2.wkey);
        const HostTensor *g = find(s2.bnprefix + ".weight"), *be = find(s2.bnprefix + ".bias"), *m = find(s2.bnprefix + ".running_mean"), *v = find(s2.bnprefix + ".running_var");
        if (!g || !be || !m || !v) return fail(GRNET_ENOENT, "missing BatchNorm tensors " + s2.bnprefix + ".*");
        if ((int)g->numel() != s2.cout) return fail(GRNET_EINVAL, "bad BatchNorm size " + s2.bnprefix);
        for (int co = 0; co < s2.cout; ++co) {
            const double sc = (double)g->data[co] / std::sqrt((double)v->data[co] + kBnEps);
            bp[co] = (float)((double)bp[co] + (double)be->data[co] - (double)m->data[co] * sc);
            for (int ci = 0; ci < cin2; ++ci) {
                const int cc = L.in.c + ci;
                wp[(((size_t)(cc / 32) * taps + 0) * L.cout_pad + co) * 32 + cc % 32] = (float)((double)w->data[(size_t)co * cin2 + ci] * sc);
            }
        }
    }
    int rc;
    if (bf) {                                              // round the folded weights to bf16 (nearest even), two per float slot
        std::vector<float> packed((wp.size() + 1) / 2, 0.f);
        uint16_t* h16 = reinterpret_cast<uint16_t*>(packed.data());
        for (size_t i = 0; i < wp.size(); ++i) h16[i] = f32_to_bf16(wp[i]);
        if ((rc = upload(packed, &L.w_dev))) return rc;
    } else if ((rc = upload(wp, &L.w_dev))) {
        return rc;
    }
    if ((rc = upload(bp, &L.b_dev))) return rc;
    if (stem) {
        std::vector<float> sw(7 * 4 * 64);
        pack_stem_weights(wfold.data(), sw.data());
        if ((rc = upload(sw, &L.stem_dev))) return rc;
    }
    if (stem_bf) {                                          // conv_bf16_stem: 4 x 64 x 8 bf16, two per float slot
        std::vector<float> sw(4 * 64 * 8 / 2);
        pack_stem_weights_bf16(wfold.data(), reinterpret_cast<unsigned short*>(sw.data()));
        if ((rc = upload(sw, &L.stem_dev))) return rc;
    }
    if (wino4s) {                                          // U = G g G^T of the folded filter, fp64 -> fp32
        std::vector<float> uws((size_t)36 * cin * L.cout);
        pack_wino4r_weights(wfold.data(), L.cout, cin, uws.data());
        if ((rc = upload(uws, &L.wino4s_dev))) return rc;
    }
    if (wino4) {
        std::vector<float> uw4((size_t)36 * L.cin_pad * L.cout_pad);
        pack_wino4_weights(wfold.data(), L.cout, cin, L.cin_pad, L.cout_pad, uw4.data(), L.in.w);
        if ((rc = upload(uw4, &L.wino4_dev))) return rc;
    }
    return 0;
}

int grnet::upload_key(const std::string& k, size_t numel, const float** d) {
    const HostTensor* t = find(k);
    if (!t) return fail(GRNET_ENOENT, "missing tensor " + k);
    if (t->numel() != numel) return fail(GRNET_EINVAL, "bad size for " + k);
    float* p = nullptr;
    int rc = upload(t->data, &p);
    *d = p;
    return rc;
}

// GRU weights are optional: loaded when every tensor is present under "gru." (standalone) or
// "pfeat_corrector.featnet." (inside a MAX-GRNet checkpoint, feature_correction.py:44).
int grnet::finalize_gru() {
    std::string pre;
    if (find("gru.rnn.weight_ih_l0")) pre = "gru.";
    else if (find("pfeat_corrector.featnet.rnn.weight_ih_l0")) pre = "pfeat_corrector.featnet.";
    else return 0;
    int rc;
    if ((rc = upload_key(pre + "cparam_mpl.weight", 128 * 3 * 24, &gruw.cparam_w))) return rc;
    for (int l = 0; l < 2; ++l)
        for (int d = 0; d < 2; ++d) {
            const std::string suf = "_l" + std::to_string(l) + (d ? "_reverse" : "");
            const size_t insz = l == 0 ? 3072 : 600;
            if ((rc = upload_key(pre + "rnn.weight_ih" + suf, 900 * insz, &gruw.w_ih[l][d]))) return rc;
            if ((rc = upload_key(pre + "rnn.bias_ih" + suf, 900, &gruw.b_ih[l][d]))) return rc;
            if ((rc = upload_key(pre + "rnn.bias_hh" + suf, 900, &gruw.b_hh[l][d]))) return rc;
            const HostTensor* whh = find(pre + "rnn.weight_hh" + suf);
            if (!whh || whh->numel() != 900 * 300) return fail(GRNET_ENOENT, "missing tensor " + pre + "rnn.weight_hh" + suf);
            std::vector<float> tr(900 * 300);
            for (int g = 0; g < 900; ++g)
                for (int k = 0; k < 300; ++k) tr[(size_t)k * 900 + g] = whh->data[(size_t)g * 300 + k];
            float* p = nullptr;
            if ((rc = upload(tr, &p))) return rc;
            gruw.w_hh[l][d] = p;
        }
    struct { const char* name; const float** w0; const float** b0; const float** w2; const float** b2; int in, out; } heads[3] = {
        {"speed_mlp", &gruw.speed_w0, &gruw.speed_b0, &gruw.speed_w2, &gruw.speed_b2, 1200, 1},
        {"step_mlp", &gruw.step_w0, &gruw.step_b0, &gruw.step_w2, &gruw.step_b2, 1200, 2},
        {"phase_mlp", &gruw.phase_w0, &gruw.phase_b0, &gruw.phase_w2, &gruw.phase_b2, 600, 4}};
    for (auto& hd : heads) {
        const std::string q = pre + hd.name;
        if ((rc = upload_key(q + ".0.weight", (size_t)100 * hd.in, hd.w0))) return rc;
        if ((rc = upload_key(q + ".0.bias", 100, hd.b0))) return rc;
        if ((rc = upload_key(q + ".2.weight", (size_t)hd.out * 100, hd.w2))) return rc;
        if ((rc = upload_key(q + ".2.bias", hd.out, hd.b2))) return rc;
    }
    gru_ready = true;
    return 0;
}

// The attention block of the pose-feature corrector is optional as well: "tsattn." (standalone) or
// "pfeat_corrector.featTencoder.0." (inside a MAX-GRNet checkpoint, feature_correction.py:95).
int grnet::finalize_tsattn() {
    std::string pre;
    if (find("tsattn.mulattn.qkv_t.weight")) pre = "tsattn.";
    else if (find("pfeat_corrector.featTencoder.0.mulattn.qkv_t.weight")) pre = "pfeat_corrector.featTencoder.0.";
    else return 0;
    const size_t D = 3072, E = 1000;
    struct { const char* key; size_t n; const float** dst; } items[] = {
        {"norm1.gamma", D, &tsw.n1_g}, {"norm1.beta", D, &tsw.n1_b}, {"norm2.gamma", D, &tsw.n2_g}, {"norm2.beta", D, &tsw.n2_b},
        {"mulattn.qkv_t.weight", 3 * E * D, &tsw.qkv_t_w}, {"mulattn.qkv_t.bias", 3 * E, &tsw.qkv_t_b},
        {"mulattn.ts_attn.weight", 4 * E * E, &tsw.ts_w}, {"mulattn.ts_attn.bias", 2 * E, &tsw.ts_b},
        {"mulattn.qkv_s.weight", 3 * E * (D + 128), &tsw.qkv_s_w}, {"mulattn.qkv_s.bias", 3 * E, &tsw.qkv_s_b},
        {"mulattn.fc_s.weight", D * E, &tsw.fc_s_w}, {"mulattn.fc_s.bias", D, &tsw.fc_s_b},
        {"mulattn.fc_t.weight", D * E, &tsw.fc_t_w}, {"mulattn.fc_t.bias", D, &tsw.fc_t_b},
        {"ffn.jwff_layer1.weight", 64 * 128 * 24, &tsw.jw1}, {"ffn.jwff_layer2.weight", 128 * 64 * 24, &tsw.jw2}};
    for (auto& it : items) {
        int rc = upload_key(pre + it.key, it.n, it.dst);
        if (rc) return rc;
    }
    tsattn_ready = true;
    return 0;
}

// The rest of the pose-feature corrector (feature_correction.py:66-91): the two gait-token MLPs and the two input BatchNorm1d
// (eval: folded to scale / shift in fp64).  Optional, under the keys of a MAX-GRNet checkpoint.
int grnet::finalize_featcorr() {
    const std::string pre = "pfeat_corrector.";
    if (!find(pre + "gfeat_mpl_t.0.weight")) return 0;
    int rc;
    if ((rc = upload_key(pre + "gfeat_mpl_t.0.weight", 1536 * 7, &fcw.t0_w))) return rc;
    if ((rc = upload_key(pre + "gfeat_mpl_t.0.bias", 1536, &fcw.t0_b))) return rc;
    if ((rc = upload_key(pre + "gfeat_mpl_t.3.weight", (size_t)3072 * 1536, &fcw.t3_w))) return rc;
    if ((rc = upload_key(pre + "gfeat_mpl_t.3.bias", 3072, &fcw.t3_b))) return rc;
    if ((rc = upload_key(pre + "gfeat_mpl_s.0.weight", 64 * 7, &fcw.s0_w))) return rc;
    if ((rc = upload_key(pre + "gfeat_mpl_s.0.bias", 64, &fcw.s0_b))) return rc;
    if ((rc = upload_key(pre + "gfeat_mpl_s.3.weight", 128 * 64, &fcw.s3_w))) return rc;
    if ((rc = upload_key(pre + "gfeat_mpl_s.3.bias", 128, &fcw.s3_b))) return rc;
    struct { const char* name; size_t c; const float** scale; const float** shift; } bns[2] = {
        {"bn_in", 3072, &fcw.bn_scale, &fcw.bn_shift}, {"bn_in_s", 3200, &fcw.bns_scale, &fcw.bns_shift}};
    for (auto& bn : bns) {
        const HostTensor *g = find(pre + bn.name + ".weight"), *be = find(pre + bn.name + ".bias"),
                         *m = find(pre + bn.name + ".running_mean"), *v = find(pre + bn.name + ".running_var");
        if (!g || !be || !m || !v) return fail(GRNET_ENOENT, "missing BatchNorm1d tensors " + pre + bn.name + ".*");
        if (g->numel() != bn.c || be->numel() != bn.c || m->numel() != bn.c || v->numel() != bn.c)
            return fail(GRNET_EINVAL, "bad BatchNorm1d size " + pre + bn.name);
        std::vector<float> sc(bn.c), sh(bn.c);
        for (size_t c = 0; c < bn.c; ++c) {
            const double k = (double)g->data[c] / std::sqrt((double)v->data[c] + kBnEps);
            sc[c] = (float)k;
            sh[c] = (float)((double)be->data[c] - (double)m->data[c] * k);
        }
        float* p = nullptr;
        if ((rc = upload(sc, &p))) return rc;
        *bn.scale = p;
        if ((rc = upload(sh, &p))) return rc;
        *bn.shift = p;
    }
    featcorr_ready = true;
    return 0;
}

// The 1x1 fuse terms of one HR module (hrnet.py:199-210: Conv2d 1x1 + BatchNorm2d; the nearest upsampling commutes with both):
// BatchNorm folded in fp64, weights in the MFMA B-fragment order of hr_fuse.hip, the shifts of an output's terms summed into one bias.
int grnet::pack_fuse_up(FuseUpPlan& fp) {
    for (int i = 0; i < fp.nb - 1; ++i) {
        if (fp.only >= 0 && fp.only != i) continue;
        const int co = kBranchCh[i];
        std::vector<double> bias(co, 0.0);
        for (int j = i + 1; j < fp.nb; ++j) {
            const int ci = kBranchCh[j];
            const std::string q = fp.prefix + "fuse_layers." + std::to_string(i) + "." + std::to_string(j) + ".";
            const HostTensor* w = find(q + "0.weight");
            if (!w) return fail(GRNET_ENOENT, "missing tensor " + q + "0.weight");
            if (w->shape.size() != 4 || w->shape[0] != co || w->shape[1] != ci || w->shape[2] != 1 || w->shape[3] != 1) return fail(GRNET_EINVAL, "bad shape for " + q + "0.weight");
            const HostTensor *g = find(q + "1.weight"), *be = find(q + "1.bias"), *m = find(q + "1.running_mean"), *v = find(q + "1.running_var");
            if (!g || !be || !m || !v) return fail(GRNET_ENOENT, "missing BatchNorm tensors " + q + "1.*");
            if ((int)g->numel() != co || (int)be->numel() != co || (int)m->numel() != co || (int)v->numel() != co) return fail(GRNET_EINVAL, "bad BatchNorm size " + q + "1");
            std::vector<double> wf((size_t)co * ci);
            for (int c = 0; c < co; ++c) {
                const double sc = (double)g->data[c] / std::sqrt((double)v->data[c] + kBnEps);
                bias[c] += (double)be->data[c] - (double)m->data[c] * sc;
                for (int k = 0; k < ci; ++k) wf[(size_t)c * ci + k] = (double)w->data[(size_t)c * ci + k] * sc;
            }
            std::vector<float> packed((size_t)co * ci / (dtype == 1 ? 2 : 1));
            if (dtype == 1) pack_fuse_up_weights_bf16(wf.data(), co, ci, reinterpret_cast<unsigned short*>(packed.data()));
            else pack_fuse_up_weights(wf.data(), co, ci, packed.data());
            if (int rc = upload(packed, &fp.w_dev[i][j - i - 1])) return rc;
        }
        std::vector<float> bf(bias.begin(), bias.end());
        if (int rc = upload(bf, &fp.b_dev[i])) return rc;
    }
    return 0;
}

int grnet::finalize() {
    if (finalized) return fail(GRNET_ESTATE, "weights already finalized");
    for (auto& L : convs) {
        int rc = pack_conv(L);
        if (rc) return rc;
    }
    for (auto& fp : fuse_ups) {
        int rc = pack_fuse_up(fp);
        if (rc) return rc;
    }
    int rc;
    {   // per-joint 128 -> 6 weights (locallyconnected2d.py:43-46), stored (6,128,24) = [o][c][j]; the tail kernel walks c with one
        // thread per (j, o): re-order to [c][j][o] so every step reads 144 contiguous floats instead of 144 lines
        const HostTensor* t = find("head.pose_mlp.weight");
        if (!t) return fail(GRNET_ENOENT, "missing tensor head.pose_mlp.weight");
        if (t->numel() != 6 * 128 * 24) return fail(GRNET_EINVAL, "bad size for head.pose_mlp.weight");
        std::vector<float> tr(6 * 128 * 24);
        for (int o = 0; o < 6; ++o)
            for (int c = 0; c < 128; ++c)
                for (int j = 0; j < 24; ++j) tr[(size_t)c * 144 + j * 6 + o] = t->data[((size_t)o * 128 + c) * 24 + j];
        float* p = nullptr;
        if ((rc = upload(tr, &p))) return rc;
        tailw.pose_w = p;
    }
    if ((rc = upload_key("head.shape_mlp.weight", 10 * 1536, &tailw.shape_w))) return rc;
    if ((rc = upload_key("head.shape_mlp.bias", 10, &tailw.shape_b))) return rc;
    if ((rc = upload_key("head.cam_mlp.weight", 3 * 1536, &tailw.cam_w))) return rc;
    if ((rc = upload_key("head.cam_mlp.bias", 3, &tailw.cam_b))) return rc;
    if ((rc = finalize_gru())) return rc;
    if ((rc = finalize_tsattn())) return rc;
    if ((rc = finalize_featcorr())) return rc;
    if (!smpl_loaded) return fail(GRNET_ESTATE, "grnet_load_smpl must be called before grnet_finalize_weights");
    tensors.clear();                                    // host copies no longer needed
    finalized = true;
    return 0;
}

extern "C" {

int grnet_load_tensor(grnet_t* h, const char* key, const void* host_ptr, const int64_t* shape, int ndim, int dtype) {
    if (!h || !key || (!host_ptr && ndim >= 0 && dtype == GRNET_DTYPE_F32) || ndim < 0 || ndim > 8) return GRNET_EINVAL;
    if (h->finalized) return h->fail(GRNET_ESTATE, "grnet_load_tensor after grnet_finalize_weights");
    if (dtype == GRNET_DTYPE_I64) return 0;                 // num_batches_tracked: irrelevant in eval
    if (dtype != GRNET_DTYPE_F32) return h->fail(GRNET_EINVAL, std::string("unsupported dtype for ") + key);
    HostTensor t;
    size_t numel = 1;
    for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); numel *= (size_t)shape[i]; }
    t.data.assign(static_cast<const float*>(host_ptr), static_cast<const float*>(host_ptr) + numel);
    h->tensors[key] = std::move(t);
    return 0;
}

int grnet_load_smpl(grnet_t* h, const float* v_template, const float* shapedirs, const float* posedirs, const float* J_regressor,
                    const float* lbs_weights, const int32_t* parents, const float* J_regressor_extra) {
    if (!h || !v_template || !shapedirs || !posedirs || !J_regressor || !lbs_weights || !parents || !J_regressor_extra)
        return GRNET_EINVAL;
    DeviceGuard guard(h->device);
    const int V = 6890;
    for (int i = 0; i < 24; ++i)
        if (parents[i] >= i || (i > 0 && parents[i] < 0)) return h->fail(GRNET_EINVAL, "SMPL parents must be topologically ordered");
    auto up = [&](const float* src, size_t n, const float** dst) {
        std::vector<float> tmp(src, src + n);
        float* p = nullptr;
        int rc = h->upload(tmp, &p);
        *dst = p;
        return rc;
    };
    int rc;
    {   // blend-shape table of the MFMA GEMM: [posedirs (207 rows) ; shapedirs^T (10) ; v_template (1) ; 0 0], row-major (220, 20670)
        const size_t C = (size_t)V * 3;
        std::vector<float> blend((size_t)kBlendK * C, 0.f);
        memcpy(blend.data(), posedirs, (size_t)207 * C * sizeof(float));
        for (size_t c = 0; c < C; ++c) {
            for (int l = 0; l < 10; ++l) blend[(size_t)(207 + l) * C + c] = shapedirs[c * 10 + l];
            blend[(size_t)217 * C + c] = v_template[c];
        }
        float* p = nullptr;
        if ((rc = h->upload(blend, &p))) return rc;
        h->smpl.blend = p;
    }
    {   // skinning weights as a padded (joint, weight) list per vertex: non-zero entries in ascending joint order
        int kmax = 1;
        for (int v = 0; v < V; ++v) {
            int c = 0;
            for (int j = 0; j < 24; ++j) c += lbs_weights[(size_t)v * 24 + j] != 0.f;
            kmax = std::max(kmax, c);
        }
        std::vector<float> w((size_t)V * kmax, 0.f), idx_f((size_t)V * kmax);
        int32_t* idx = reinterpret_cast<int32_t*>(idx_f.data());
        for (int v = 0; v < V; ++v) {
            int c = 0;
            for (int j = 0; j < 24; ++j) {
                const float wj = lbs_weights[(size_t)v * 24 + j];
                if (wj != 0.f) { idx[(size_t)v * kmax + c] = j; w[(size_t)v * kmax + c] = wj; ++c; }
            }
            for (; c < kmax; ++c) idx[(size_t)v * kmax + c] = -1;
        }
        float* p = nullptr;
        if ((rc = h->upload(w, &p))) return rc;
        h->smpl.skin_w = p;
        if ((rc = h->upload(idx_f, &p))) return rc;          // int32 payload moved as raw 4-byte words
        h->smpl.skin_idx = reinterpret_cast<const int*>(p);
        h->smpl.skin_k = kmax;
    }
    if ((rc = up(lbs_weights, (size_t)V * 24, &h->smpl.lbs_weights))) return rc;
    {   // the one extra joint the path uses (smpl.py:117: JOINT_MAP 'Thorax (MPII)' = 50 -> row 5): sparse row
        std::vector<float> w, idx_f;
        for (int v = 0; v < V; ++v) {
            const float x = J_regressor_extra[(size_t)5 * V + v];
            if (x != 0.f) { w.push_back(x); int32_t i = v; float f; memcpy(&f, &i, 4); idx_f.push_back(f); }
        }
        h->smpl.thorax_n = (int)w.size();
        if (w.empty()) { w.push_back(0.f); idx_f.push_back(0.f); }
        float* p = nullptr;
        if ((rc = h->upload(w, &p))) return rc;
        h->smpl.thorax_w = p;
        if ((rc = h->upload(idx_f, &p))) return rc;
        h->smpl.thorax_idx = reinterpret_cast<const int*>(p);
    }
    {   // all 9 rows of J_regressor_extra as one (vertex, weight) list with row offsets: the 49-joint SPIN skeleton of grnet_smooth_pose (smpl.py:119-121)
        std::vector<float> w, idx_f;
        for (int r = 0; r < 9; ++r) {
            h->smpl.extra_ptr[r] = (int)w.size();
            for (int v = 0; v < V; ++v) {
                const float x = J_regressor_extra[(size_t)r * V + v];
                if (x != 0.f) { w.push_back(x); int32_t i = v; float f; memcpy(&f, &i, 4); idx_f.push_back(f); }
            }
        }
        h->smpl.extra_ptr[9] = (int)w.size();
        if (w.empty()) { w.push_back(0.f); idx_f.push_back(0.f); }
        float* p = nullptr;
        if ((rc = h->upload(w, &p))) return rc;
        h->smpl.extra_w = p;
        if ((rc = h->upload(idx_f, &p))) return rc;
        h->smpl.extra_idx = reinterpret_cast<const int*>(p);
    }
    // the joint regressor is linear: apply it to the tables once, in fp64
    std::vector<float> Jt(72), Js(720);
    for (int j = 0; j < 24; ++j)
        for (int d = 0; d < 3; ++d) {
            double a = 0;
            double s[10] = {0};
            for (int v = 0; v < V; ++v) {
                const double w = J_regressor[(size_t)j * V + v];
                if (w == 0.0) continue;
                a += w * v_template[v * 3 + d];
                for (int l = 0; l < 10; ++l) s[l] += w * shapedirs[((size_t)v * 3 + d) * 10 + l];
            }
            Jt[j * 3 + d] = (float)a;
            for (int l = 0; l < 10; ++l) Js[(j * 3 + d) * 10 + l] = (float)s[l];
        }
    float* p = nullptr;
    if ((rc = h->upload(Jt, &p))) return rc;
    h->smpl.J_template = p;
    if ((rc = h->upload(Js, &p))) return rc;
    h->smpl.J_shapedirs = p;
    void* q = nullptr;
    if (hipMalloc(&q, 24 * sizeof(int)) != hipSuccess) return h->fail(GRNET_ENOMEM, "hipMalloc failed");
    h->dev_allocs.push_back(q);
    if (hipMemcpy(q, parents, 24 * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) return h->fail(GRNET_EHIP, "hipMemcpy failed");
    h->smpl.parents = static_cast<const int*>(q);
    h->smpl_loaded = true;
    return 0;
}

int grnet_finalize_weights(grnet_t* h) {
    if (!h) return GRNET_EINVAL;
    DeviceGuard guard(h->device);
    return h->finalize();
}

// VPRegressor.forward's J_regressor override -- lib/models/pare.py:70-76.  The selection ([:, H36M_TO_J14]) is applied to the table's rows here,
// so the kernel computes the surviving rows only.
int grnet_set_joint_regressor(grnet_t* h, const float* J_host, int rows, const int32_t* select, int n_select) {
    if (!h) return GRNET_EINVAL;
    DeviceGuard guard(h->device);
    if (!J_host) { h->jreg_clear(); return 0; }
    if (rows < 1) return h->fail(GRNET_EINVAL, "joint regressor: rows must be >= 1");
    if (select && n_select < 1) return h->fail(GRNET_EINVAL, "joint regressor: an empty selection");
    const int jout = select ? n_select : rows;
    if (jout > kJregMaxRows)
        return h->fail(GRNET_EINVAL, "joint regressor: " + std::to_string(jout) + " output rows exceed the limit of " + std::to_string(kJregMaxRows));
    const size_t V = 6890;
    std::vector<float> W((size_t)jout * V);
    for (int j = 0; j < jout; ++j) {
        const int r = select ? select[j] : j;
        if (r < 0 || r >= rows)
            return h->fail(GRNET_EINVAL, "joint regressor: selected row " + std::to_string(r) + " is outside [0, " + std::to_string(rows) + ")");
        const float* src = J_host + (size_t)r * V;
        for (size_t v = 0; v < V; ++v) {
            if (!std::isfinite(src[v]))
                return h->fail(GRNET_EINVAL, "joint regressor: non-finite entry in row " + std::to_string(r) + ", column " + std::to_string(v));
            W[(size_t)j * V + v] = src[v];
        }
    }
    std::vector<float> pack(joint_regress_pack_floats(jout));
    joint_regress_pack(W.data(), jout, pack.data());
    void *p = nullptr, *ws = nullptr;                      // allocate and fill first: a failure leaves the earlier table in place, like a refusal
    if (hipMalloc(&p, pack.size() * sizeof(float)) != hipSuccess ||
        hipMalloc(&ws, joint_regress_workspace_floats(jout, h->max_frames) * sizeof(float)) != hipSuccess) {
        if (p) (void)hipFree(p);
        return h->fail(GRNET_ENOMEM, "joint regressor: hipMalloc of the table / workspace failed");
    }
    hipError_t e = hipMemcpy(p, pack.data(), pack.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(p); (void)hipFree(ws);
        return h->fail(GRNET_EHIP, std::string("joint regressor upload: ") + hipGetErrorString(e));
    }
    h->jreg_clear();
    h->jreg_pack = static_cast<float*>(p);
    h->jreg_ws = static_cast<float*>(ws);
    h->jreg_rows = jout;
    return 0;
}

}  // extern "C"
