// The handle on its device: allocation, the choice of a kernel per convolution and call size, the launch path of a forward (eager on the lane
// streams or as a replayed hipGraph), the tuner, and the tail passes of the temporal branch.  Every function that runs once per op of a forward
// is in this file or inline in grnet_impl.h: a step is ~300 launches, and none of them crosses a translation unit on the host.
#include "grnet_impl.h"

namespace grk { thread_local GraphRecorder* g_recorder = nullptr; }

int grnet::allocate() {
    // 64 floats of leading zero block, 256-byte aligned buffers (one after the other, or shared by liveness: plan_arena), 256 bytes of tail:
    // conv_wino4s_f32's 16-byte row loads on 7-wide maps touch (and mask) one float past a row, i.e. 4 bytes past the LAST buffer's end
    // for its last row -- they stay inside the arena (in a compact one such a masked read may land in another tenant's bytes)
    if (plan_arena(compact, arena_plan)) return fail(GRNET_ESTATE, "the activation arena could not be planned: a launch group or the assignment violates the sharing rule");
    const size_t total = (size_t)arena_plan.total;
    arena_floats = total;
    void* q = nullptr;
    if (hipMalloc(&q, total * sizeof(float)) != hipSuccess)
        return fail(GRNET_ENOMEM, std::string("hipMalloc of the ") + (compact ? "compact " : "") + "activation arena (" + std::to_string(total * 4 >> 20) + " MiB) failed");
    arena = static_cast<float*>(q);
    if (hipMemset(arena, 0, 64 * sizeof(float)) != hipSuccess) return fail(GRNET_EHIP, "hipMemset failed");
    zeros = arena;
    // streams / events of the parallel lanes are created here, never inside a stream capture
    if (hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming) != hipSuccess) return fail(GRNET_EHIP, "hipEventCreate failed");
    if (int rc = install_schedule(max_frames)) return rc;
    if (hipStreamCreateWithFlags(&capture_stream, hipStreamNonBlocking) != hipSuccess) return fail(GRNET_EHIP, "hipStreamCreate failed");
    const size_t n = max_frames;
    int rc;
    if ((rc = dev_alloc(&d_plf, n * 128 * 24))) return rc;
    if ((rc = dev_alloc(&d_csf, n * 64 * 24))) return rc;
    if ((rc = dev_alloc(&d_stats, softmax_pool_ws_floats((int)n)))) return rc;
    if ((rc = dev_alloc(&d_rot6d, n * 144))) return rc;
    if ((rc = dev_alloc(&d_shape, n * 10))) return rc;
    if ((rc = dev_alloc(&d_cam, n * 3))) return rc;
    if ((rc = dev_alloc(&d_rotmat, n * 216))) return rc;
    if ((rc = dev_alloc(&d_theta, n * 85))) return rc;
    if ((rc = dev_alloc(&d_A, n * kSmplWsFloatsPerFrame))) return rc;
    if ((rc = dev_alloc(&d_verts, n * 6890 * 3))) return rc;
    if ((rc = dev_alloc(&d_kp3d, n * 87))) return rc;
    if ((rc = dev_alloc(&d_kp2d, n * 58))) return rc;
    return 0;
}

// Build ops_flat from the plan: lane placement, cross-lane events, the streams the schedule uses.
// (Round 4 also re-placed the lanes at tune time from the durations grnet_op_timeline measures in company: 3.728 -> 3.784 ms and
// 3.735 -> 3.757 ms per step, i.e. no better than the calibrated estimates below; removed.)
int grnet::install_schedule(int n) {
    drop_graphs();
    seen_once.clear();
    for (hipEvent_t e : op_events_flat) if (e) (void)hipEventDestroy(e);
    op_events_flat.clear();
    ops_flat = ops;
    static const int sched_env = GRNET_AB(LANE_SCHED, 1);   // 0: lanes as written in the plan
    if (sched_env) schedule_lanes(ops_flat, n);
    analyze_dependencies(ops_flat, op_events_flat);
    int used = 1;                                          // only the streams the schedule really uses are forked / joined
    for (const Op& op : ops_flat) used = std::max(used, op.lane + 1);
    for (int l = 1; l < used; ++l) {
        if (!side[l] && hipStreamCreateWithFlags(&side[l], hipStreamNonBlocking) != hipSuccess) return fail(GRNET_EHIP, "hipStreamCreate failed");
        if (!ev_join[l] && hipEventCreateWithFlags(&ev_join[l], hipEventDisableTiming) != hipSuccess) return fail(GRNET_EHIP, "hipEventCreate failed");
    }
    lanes_used = used;
    for (size_t i = 0; i < ops_flat.size(); ++i)
        if (ops_flat[i].record && hipEventCreateWithFlags(&op_events_flat[i], hipEventDisableTiming) != hipSuccess)
            return fail(GRNET_EHIP, "hipEventCreate failed");
    return 0;
}

// ------------------------------------------------------------------ the kernel choice
int grnet::hint_for(const ConvLayer& L, int n) const {
    if (conv_tile_hint) return conv_tile_hint;
    auto m = tuned_mode.find(n);
    if (m == tuned_mode.end() || !(m->second & 1)) return 0;      // cost model
    auto it = L.tuned.find(n);
    return it == L.tuned.end() ? 0 : it->second;
}

// conv_wino4s_f32 on this layer in a call of n frames?  A 7x7 row tile is four images: below three row tiles (n < 12) a launch is
// 16-32 workgroups whose waves each walk 16 k-steps, and the direct split-K kernel with its 8-wave workgroups is the shorter chain
// link (measured at 1 / 2 / 4 / 8 / 12 frames: -4 % / -3 % / -5 % / -4 % / +0.5 % with the 7x7 layers on it; 14x14: +2 ... +4 % throughout)
bool grnet::wino4s_runs(const ConvLayer& L, int n) const { return L.wino4s_dev && wino_mode && (L.in.w != 7 || n >= 12); }
// layer1's 64 -> 256 1x1 convolutions and the PARE head's 128 -> 25 heat-map layer on 56x56 maps: the register-resident kernel of
// conv_pw.hip (fp32 handles; GRNET_PW: bit 0 64 -> 256, bit 1 128 -> 25, bit 2 the rest of the eligible shapes -- 64 -> 64 and
// 128 -> 64 measure within 1 us of the generic kernel either way and stay on it; 0: the generic kernel everywhere)
bool grnet::pw_on(const ConvLayer& L) const {
    static const int pw_env = GRNET_AB(PW, 3);
    return dtype == 0 && L.in.w == 56 && L.segs.size() == 1 && L.cin_w == L.in.c && (L.adds.empty() || L.adds[0].shift == 0) &&
           conv_pw_eligible(L.in.c, L.cout, L.ks, L.stride, L.in.h, L.in.w, (int)L.adds.size()) && L.cout_pad >= (L.cout > 32 ? (L.cout + 63) / 64 * 64 : 32) &&
           (pw_env & (L.in.c == 64 && L.cout >= 128 ? 1 : L.in.c == 128 && L.cout <= 32 ? 2 : 4));
}
// The smallest call of a bf16 kernel group: its own default, or what GRNET_OPT_BF16_MIN_FRAMES sets for all of them
int grnet::bf16_from(int dflt) const { return bf16_min_frames ? bf16_min_frames : dflt; }
// bf16: does chain `c` run as ONE conv_bf16_chain launch in a call of n frames?  A chain workgroup is one frame on one CU: from about a
// quarter of the chip's CUs on it beats eight launches (GRNET_BF16_CHAIN: bit 0 64 ch @28x28, bit 1 128 ch @14x14, bit 2 256 ch @7x7, bit 3 32 ch @56x56 --
// there a launch per BasicBlock with 19-row bands resident;
// GRNET_BF16_CHAIN_MIN: smallest call that takes it).  A forced tile (tests / tuning) switches it off like every special kernel.
bool grnet::chain_active(const ChainPlan& c, int n) const {
    return dtype == 1 && !conv_tile_hint && n >= bf16_from(64) && (chain_mode & (c.w == 28 ? 1 : c.w == 14 ? 2 : c.w == 7 ? 4 : 8));
}
// bf16: the wide 3x3 stride-1 layers (upsample heads, PARE head, layer1's 3x3) on conv_bf16_wide_band.  A workgroup is a band of 7 / 14 rows of one
// frame x 128 (64) output channels: from 32 frames per call on a launch has at least one workgroup per CU (bit 4 of the GRNET_OPT_BF16_CHAIN mask;
// GRNET_BF16_WIDE_MIN: smallest call).  A forced tile switches it off like every special kernel.
bool grnet::wide_runs(const ConvLayer& L, int n) const {
    if (dtype != 1 || !(chain_mode & 16) || conv_tile_hint || n < bf16_from(32) || L.stem_dev || !L.w_dev) return false;
    return conv_bf16_wide_eligible(conv_args(L, nullptr, n));
}
// bf16: the 3x3 stride-2 layers (fuse-layer down paths, transitions, the stem's second convolution) on conv_bf16_s2_band, from 64 frames per call on
// (a workgroup is a band of one frame; GRNET_BF16_S2_MIN).  Bit 5 of the GRNET_OPT_BF16_CHAIN mask.
bool grnet::s2_runs(const ConvLayer& L, int n) const {
    if (dtype != 1 || !(chain_mode & 32) || conv_tile_hint || n < bf16_from(64) || L.stem_dev || !L.w_dev || L.in2.c) return false;
    return conv_bf16_s2_eligible(conv_args(L, nullptr, n));
}
// bf16: the stem pair (bit 9 of the mask) / a layer1 Bottleneck (bit 8) as ONE row-walking launch (conv_bf16_roll.hip), from 64 frames per call on (a workgroup is a
// frame, or a quarter of one): HBM sees the launch's input and output once.  A forced tile switches it off like every special kernel.
bool grnet::roll_active(const RollPlan& r, int n) const {
    return dtype == 1 && !conv_tile_hint && n >= bf16_from(64) && (chain_mode & (r.kind == 0 ? 512 : 256));
}
grnet::ConvKernel grnet::kernel_for(const ConvLayer& L, int n) const {
    static const int w4s_env = GRNET_AB(WINO4S, 7);      // bit 0: 128 @14x14, bit 1: 256 @7x7, bit 2: 256 @14x14
    if (dtype == 1 && L.roll >= 0 && roll_active(rolls[L.roll], n)) return L.roll_pos == 0 ? K_BF16_ROLL : K_BF16_ROLL_MEMBER;
    if (dtype == 1 && L.chain >= 0 && chain_active(chains[L.chain], n)) return L.chain_pos == 0 ? K_BF16_CHAIN : K_BF16_CHAIN_MEMBER;
    if (dtype == 1 && L.pair_next >= 0 && pair_active(n)) return K_BF16_PAIR;
    if (dtype == 1 && L.pair_of >= 0 && pair_active(n)) return K_BF16_PAIR_MEMBER;
    if (dtype == 1 && wide_runs(L, n)) return K_BF16_WIDE;
    if (dtype == 1 && s2_runs(L, n)) return K_BF16_S2;
    if (dtype == 1) return L.stem_dev ? K_BF16_STEM : K_BF16;      // (a plan built for conv_bf16_stem has no NHWC copy of the frames for the generic kernel)
    if (conv_tile_hint) return K_DIRECT;                   // a forced tile also switches every special kernel off (tests / tuning)
    if (wino4s_runs(L, n) && (w4s_env & (L.in.w == 7 ? 2 : L.in.c == 128 ? 1 : 4))) return K_WINO4S;
    if (pw_on(L)) return K_PW;
    if (L.stem_dev) return K_STEM;
    if (L.wino4_dev && wino_mode) return K_WINO4;
    return K_DIRECT;
}
// multiplies the matrix cores execute per algorithmic multiply of L: F(4x4,3x3) does 36 per 4x4 tile instead of 144; the small maps pay
// for their padding (14 -> 16, 7 -> 8 per side)
double grnet::executed_ratio(const ConvLayer& L, int n) const {
    switch (kernel_for(L, n)) {
        case K_WINO4S: return 0.25 * (L.in.w == 14 ? 256.0 / 196.0 : 64.0 / 49.0);
        case K_WINO4: return 0.25;
        default: return 1.0;
    }
}
std::string grnet::kernel_name(const ConvLayer& L, int n) const {
    char b[96];
    switch (kernel_for(L, n)) {
        case K_BF16: return "conv_bf16";
        case K_BF16_STEM: return "conv_bf16_stem";
        case K_BF16_ROLL: return rolls[L.roll].kind == 0 ? "conv_bf16_stem_pair" : "conv_bf16_bneck";
        case K_BF16_ROLL_MEMBER: return rolls[L.roll].kind == 0 ? "conv_bf16_stem_pair+" : "conv_bf16_bneck+";      // runs inside the launch of the group's first member
        case K_BF16_PAIR: return "conv_bf16_pair";
        case K_BF16_PAIR_MEMBER: return "conv_bf16_pair+";     // runs inside the pair's launch
        case K_BF16_WIDE: snprintf(b, sizeof b, "conv_bf16_wide<%d,%d>", L.in.c >= 128 ? 128 : 64, L.in.w); return b;
        case K_BF16_S2: snprintf(b, sizeof b, "conv_bf16_s2<%d>", L.out.w); return b;
        case K_BF16_CHAIN: snprintf(b, sizeof b, "conv_bf16_chain<%d,%d>", L.in.c, L.in.w); return b;
        case K_BF16_CHAIN_MEMBER: snprintf(b, sizeof b, "conv_bf16_chain<%d,%d>+", L.in.c, L.in.w); return b;      // runs inside the chain's launch: no launch, no time of its own
        case K_WINO4S: snprintf(b, sizeof b, "conv_wino4s_f32<%d,%d>", L.in.w, L.in.c); return b;
        case K_PW: snprintf(b, sizeof b, "conv_pw_f32<%d>", L.in.c); return b;
        case K_STEM: return "conv_stem_f32";
        case K_WINO4: {
            const int npw = conv_wino4_wide(L.cout, L.in.w);
            if (npw && L.cin_pad % 16 == 0 && L.cout_pad % (npw * 32) == 0) snprintf(b, sizeof b, "conv_wino4w_f32<%d,%d>", L.in.w, npw);
            else snprintf(b, sizeof b, "conv_wino4_f32<%d,%d>", conv_wino4_blocks(L.cout, L.in.w), L.in.w);
            return b;
        }
        default: snprintf(b, sizeof b, "conv_direct_f32 %dx%d s%d", L.ks, L.ks, L.stride); return b;
    }
}
// grnet_conv_launch_form: what a call of n frames launches for L under the hint in effect, from the launchers' own choice functions
// (conv_choose, conv_wino4_form, conv_wino4s_images_per_tile).  fp32 handles.
int grnet::launch_form(const ConvLayer& L, int n, std::string* out) {
    char b[192];
    ConvArgs a = conv_args(L, nullptr, n);
    switch (kernel_for(L, n)) {
        case K_WINO4S: {
            const int ipw = conv_wino4s_images_per_tile(L.in.w);
            int last = 0;
            const int tiles = conv_wino4s_row_tiles(L.in.w, n, &last);
            snprintf(b, sizeof b, "wino4s images_per_tile=%d row_tiles=%d partial=%d", ipw, tiles, last < ipw ? 1 : 0);
            break;
        }
        case K_PW: snprintf(b, sizeof b, "pw"); break;
        case K_STEM: snprintf(b, sizeof b, "stem"); break;
        case K_WINO4: {
            Wino4Form f;
            if (conv_wino4_form(a, &f) != hipSuccess) return fail(GRNET_EINVAL, "no F(4x4,3x3) launch for " + L.segs[0].wkey);
            if (f.waves == 8) snprintf(b, sizeof b, "wino4w waves=8 npw=%d gx=%d gy=%d xcd=%d split=0", f.npw, f.gx, f.gy, f.xcd);
            else snprintf(b, sizeof b, "wino4 waves=4 nb=%d gx=%d gy=%d xcd=%d split=%d full=%d rest=%d", f.nb, f.gx, f.gy, f.xcd, f.split, f.full, f.rest);
            break;
        }
        case K_DIRECT: {
            const int hint = hint_for(L, n);
            ConvChoice c;
            if (conv_choose(a, hint, &c) != hipSuccess)
                return fail(GRNET_EINVAL, "tile hint " + std::to_string(hint) + " is not valid for " + L.segs[0].wkey + " at " + std::to_string(n) + " frames");
            snprintf(b, sizeof b, "direct split_k=%d pixel_tile=%d channel_tile=%d waves=%d width_variant=%d rows=%d hint=%d", c.family, c.tps * 16, c.tcs * 16,
                     c.waves, c.width_variant, c.rows, hint);
            break;
        }
        default: return fail(GRNET_ESTATE, "not an fp32 launch");
    }
    *out = b;
    return 0;
}
// grnet_debug_tensor: did the last forward write view v to memory?  A convolution inside a row-walking or chain launch (conv_bf16_roll.hip, conv_bf16_chain.hip)
// keeps its output in LDS unless it is the group's last one; the buffer then holds whatever an earlier forward left there.  (The pair's member writes its output.)
bool grnet::tap_written(const View& v) const {
    for (const ConvLayer& L : convs) {
        if (L.out.slot != v.slot || L.out.coff != v.coff || L.out.c != v.c) continue;
        switch (kernel_for(L, last_n)) {
            case K_BF16_ROLL: case K_BF16_ROLL_MEMBER: return L.roll_pos == (int)rolls[L.roll].convs.size() - 1;
            case K_BF16_CHAIN: case K_BF16_CHAIN_MEMBER: return L.chain_pos == (int)chains[L.chain].convs.size() - 1;
            default: return true;
        }
    }
    return true;
}

// ------------------------------------------------------------------ execution
ConvArgs grnet::conv_args(const ConvLayer& L, const float* frames, int n) const {
    ConvArgs a{};
    bind(L.in, a.in, a.in_ctot, a.in_coff, frames);
    a.N = n; a.Cin = L.in.c; a.H = L.in.h; a.W = L.in.w;
    bind(L.out, a.out, a.out_ctot, a.out_coff);
    a.Cout = L.cout; a.Ho = L.out.h; a.Wo = L.out.w;
    a.w = L.w_dev; a.bias = L.b_dev; a.CinPad = L.cin_pad; a.CoutPad = L.cout_pad;
    a.ks = L.ks; a.stride = L.stride; a.relu = L.relu; a.relu_from = L.relu_from;
    a.n_add = (int)L.adds.size();
    for (int k = 0; k < a.n_add; ++k) {
        bind(L.adds[k].v, a.add[k], a.add_ctot[k], a.add_coff[k]);
        a.add_shift[k] = L.adds[k].shift;
    }
    a.zeros = zeros;
    a.pw_stream = !(chain_mode & 128) ? 0 : bf16_min_frames ? 2 : 1;
    if (L.in2.c) { bind(L.in2, a.in2, a.in2_ctot, a.in2_coff); a.cin_split = L.in.c; a.Cin = L.in.c + L.in2.c; }
    if (L.pair_next >= 0 && pair_active(n)) {
        const ConvLayer& F = convs[L.pair_next];
        a.w2 = F.w_dev; a.bias2 = F.b_dev; bind(F.out, a.out2, a.out2_ctot, a.out2_coff); a.relu2 = F.relu;
    }
    return a;
}
int grnet::launch_conv_op(const ConvLayer& L, const float* frames, int n, hipStream_t s, int* n_launches) {
    static const int w4s_ks = GRNET_AB(WINO4S_KS, 0);
    *n_launches = 1;
    switch (kernel_for(L, n)) {
        case K_BF16: HIP_TRY(launch_conv_bf16(conv_args(L, frames, n), s, hint_for(L, n))); break;
        case K_BF16_STEM: HIP_TRY(launch_conv_bf16_stem(frames, L.stem_dev, L.b_dev, base(L.out), L.out.ctot, L.out.coff, n, L.relu, s)); break;
        case K_BF16_CHAIN: {
            const ChainPlan& cp = chains[L.chain];
            const ConvLayer& last = convs[cp.convs.back()];
            ChainArgs ca{};
            bind(L.in, ca.in, ca.in_ctot, ca.in_coff);
            bind(last.out, ca.out, ca.out_ctot, ca.out_coff);
            ca.N = n; ca.nconv = (int)cp.convs.size();
            for (int i = 0; i < ca.nconv; ++i) { ca.w[i] = convs[cp.convs[i]].w_dev; ca.bias[i] = convs[cp.convs[i]].b_dev; }
            for (int k = 0; k + 1 < ca.nconv / 2; ++k)            // the 56x56 branch runs one launch per BasicBlock: the blocks' own output buffers carry the hand-over
                bind(convs[cp.convs[2 * k + 1]].out, ca.mid[k], ca.mid_ctot[k], ca.mid_coff[k]);
            HIP_TRY(launch_conv_bf16_chain(ca, cp.c, cp.w, s));
            *n_launches = conv_bf16_chain_launches(cp.c, cp.w, ca.nconv);
            break;
        }
        case K_BF16_CHAIN_MEMBER: *n_launches = 0; break;       // its work is in the launch of the chain's first member
        case K_BF16_ROLL: {
            const RollPlan& rp = rolls[L.roll];
            const ConvLayer& last = convs[rp.convs.back()];
            if (rp.kind == 0) {
                const ConvLayer& c2 = convs[rp.convs[1]];
                HIP_TRY(launch_conv_bf16_stem_pair(frames, base(last.out), last.out.ctot, last.out.coff, n, L.stem_dev, L.b_dev, c2.w_dev, c2.b_dev, s));
            } else {
                const ConvLayer &c2 = convs[rp.convs[1]], &c3 = convs[rp.convs[2]];
                HIP_TRY(launch_conv_bf16_bneck(base(L.in), L.in.ctot, L.in.coff, base(last.out), last.out.ctot, last.out.coff, n, rp.kind == 1, L.w_dev, L.b_dev, c2.w_dev, c2.b_dev,
                                               c3.w_dev, c3.b_dev, s));
            }
            break;
        }
        case K_BF16_ROLL_MEMBER: *n_launches = 0; break;        // its work is in the launch of the group's first member
        case K_BF16_PAIR: HIP_TRY(launch_conv_bf16(conv_args(L, frames, n), s, 0)); break;
        case K_BF16_PAIR_MEMBER: *n_launches = 0; break;        // its work is the second stage of the expansion's launch
        case K_BF16_WIDE: HIP_TRY(launch_conv_bf16_wide(conv_args(L, frames, n), s)); break;
        case K_BF16_S2: HIP_TRY(launch_conv_bf16_s2(conv_args(L, frames, n), s)); break;
        case K_WINO4S: {
            ConvArgs wa = conv_args(L, frames, n);
            wa.w = L.wino4s_dev;
            static const int w4s_prio = GRNET_AB(WINO4S_PRIO, 3);   // bit 0: 14x14 layers, bit 1: 7x7 layers at wave priority 1
            wa.prio = (w4s_prio & (L.in.w == 7 ? 2 : 1)) ? 1 : 0;
            HIP_TRY(launch_conv_wino4s(wa, s, w4s_ks));
            break;
        }
        case K_PW: HIP_TRY(launch_conv_pw(conv_args(L, frames, n), s)); break;
        case K_STEM: {
            ConvArgs wa = conv_args(L, frames, n);
            wa.w = L.stem_dev;
            HIP_TRY(launch_conv_stem(wa, s));
            break;
        }
        case K_WINO4: {
            ConvArgs wa = conv_args(L, frames, n);
            wa.w = L.wino4_dev;
            static const int chain_prio4 = GRNET_AB(WINO_PRIO, 1);
            // the BasicBlock chains of the 56x56 and 28x28 HR branches (32-channel workgroups): wave priority 1.  Worth +1 % when
            // only the 56x56 chain ran on a Winograd kernel; with both on F(4x4,3x3) every combination is within 0.5 %
            wa.prio = (L.in.c == L.cout && L.cout <= 64 && !L.solo) ? chain_prio4 : 0;
            HIP_TRY(launch_conv_wino4(wa, s, n_launches));
            break;
        }
        case K_DIRECT: HIP_TRY(launch_conv(conv_args(L, frames, n), s, hint_for(L, n))); break;
    }
    return 0;
}
int grnet::launch_fuse_up_op(const FuseUpPlan& fp, int n, hipStream_t s) {
    FuseUpArgs a{};
    a.N = n; a.nb = fp.nb; a.only = fp.only;
    for (int i = 0; i < fp.nb - 1; ++i) {
        if (fp.only >= 0 && fp.only != i) continue;
        FuseUpOut& fo = a.o[i];
        bind(fp.outs[i], fo.out, fo.out_ctot, fo.out_coff);
        bind(fp.xs[i], fo.base, fo.base_ctot, fo.base_coff);
        fo.bias = fp.b_dev[i];
        fo.relu = 1;
        fo.n_extra = (int)fp.extra[i].size();
        for (int k = 0; k < fo.n_extra; ++k) bind(fp.extra[i][k], fo.extra[k], fo.extra_ctot[k], fo.extra_coff[k]);
        for (int j = i + 1; j < fp.nb; ++j) {
            FuseUpSrc& src = fo.src[j - i - 1];
            bind(fp.xs[j], src.x, src.ctot, src.coff);
            src.w = fp.w_dev[i][j - i - 1];
        }
    }
    HIP_TRY(dtype == 1 ? launch_hr_fuse_up_bf16(a, s) : launch_hr_fuse_up(a, s));
    return 0;
}

// The tail's outputs of one call: the caller's buffer where it gave one, else the handle's own
grnet::HeadOutputs grnet::head_outputs(const grnet_outputs_t& o) const {
    return {o.pred_rot6d ? o.pred_rot6d : d_rot6d, o.rotmat ? o.rotmat : d_rotmat, o.theta ? o.theta : d_theta,
            o.verts ? o.verts : d_verts,           o.kp_3d ? o.kp_3d : d_kp3d,     o.kp_2d ? o.kp_2d : d_kp2d};
}

int grnet::enqueue(const float* frames, int n, const grnet_outputs_t& o, hipStream_t s, bool convs_only) {
    int launches = 0;
    last_n = n;
    float* plf = o.point_local_feat ? o.point_local_feat : d_plf;
    float* csf = o.cam_shape_feats ? o.cam_shape_feats : d_csf;
    const auto [rot6d, rotmat, theta, verts, kp3d, kp2d] = head_outputs(o);
    const std::vector<Op>& ops = ops_flat;
    const std::vector<hipEvent_t>& op_events = op_events_flat;
    GraphRecorder* rec = g_recorder;                          // non-null: build graph nodes instead of launching
    const bool lanes = multi_lane && !rec;
    std::vector<hipGraphNode_t> lane_last(kLanes, nullptr), op_node(rec ? ops.size() : 0, nullptr);
    hipStream_t lane_stream[kLanes];
    for (int l = 0; l < kLanes; ++l) lane_stream[l] = s;
    if (lanes) {
        HIP_TRY(hipEventRecord(ev_fork, s));                 // fork: side lanes start after everything before this forward
        for (int l = 1; l < lanes_used; ++l) {
            lane_stream[l] = side[l];
            HIP_TRY(hipStreamWaitEvent(side[l], ev_fork, 0));
        }
    }
    hipStream_t caller = s;
    for (size_t oi = 0; oi < ops.size(); ++oi) {
        const Op& op = ops[oi];
        s = lane_stream[op.lane];
        const int lane = multi_lane ? op.lane : 0;
        if (lanes)
            for (int w : op.waits) HIP_TRY(hipStreamWaitEvent(s, op_events[w], 0));
        if (convs_only && op.kind != Op::CONV && op.kind != Op::FUSEUP) {   // a skipped op keeps its place in the order: later ops of its lane rely on its waits
            if (lanes && op.record) HIP_TRY(hipEventRecord(op_events[oi], s));
            continue;
        }
        if (tl_start && !rec) HIP_TRY(hipEventRecord((*tl_start)[oi], s));
        if (rec) {                                            // dependencies: previous node of the lane + cross-lane producers
            rec->deps.clear();
            rec->n_chain = lane_last[lane] ? 1 : 0;
            if (lane_last[lane]) rec->deps.push_back(lane_last[lane]);
            if (multi_lane)
                for (int w : op.waits)                          // several waited ops can be ONE node (the members of a chain launch): an edge is added once
                    if (op_node[w] && std::find(rec->deps.begin(), rec->deps.end(), op_node[w]) == rec->deps.end()) rec->deps.push_back(op_node[w]);
        }
        // timing-only ablation (results are garbage): GRNET_ABL_SKIP=<substring of a weight key>[,<substring>...] drops the matching
        // convolution launches and "fuse_up" the grouped fuse launches, events and dependencies stay -- what is a group of launches worth?
        static const char* abl_skip = GRNET_AB_STR(ABL_SKIP);          // diagnostic builds only (make ABLATION=1): a stray variable must not make the product drop launches
        if (abl_skip && (op.kind == Op::CONV || op.kind == Op::FUSEUP)) {
            const std::string lbl = op_label(op);
            bool skip = false;
            for (const char* q = abl_skip; *q;) {
                const char* e = strchr(q, ',');
                const std::string pat = e ? std::string(q, e) : std::string(q);
                if (!pat.empty() && lbl.find(pat) != std::string::npos) skip = true;
                q = e ? e + 1 : q + strlen(q);
            }
            if (skip) {
                if (tl_end && !rec) HIP_TRY(hipEventRecord((*tl_end)[oi], s));
                if (lanes && op.record) HIP_TRY(hipEventRecord(op_events[oi], s));
                continue;
            }
        }
        switch (op.kind) {
            case Op::CONVERT:
                HIP_TRY(launch_nchw_f32_to_nhwc_bf16(frames, base(v_in8), n, 3, 224, 224, 8, s));
                ++launches;
                break;
            case Op::CONV: {
                int nl = 1;
                if (int rc = launch_conv_op(convs[op.conv_idx], frames, n, s, &nl)) return rc;
                launches += nl;
                break;
            }
            case Op::SUM: {
                const auto& sv = sum_views[op.conv_idx];
                SumArgs a = op.sum;
                a.N = n;
                bind(sv.out, a.out, a.out_ctot, a.out_coff);
                for (int k = 0; k < a.n_add; ++k) {
                    bind(sv.adds[k].v, a.add[k], a.add_ctot[k], a.add_coff[k]);
                    a.add_shift[k] = sv.adds[k].shift;
                }
                if (dtype == 1) HIP_TRY(launch_fuse_sum_bf16(a, s));
                else HIP_TRY(launch_fuse_sum(a, s));
                ++launches;
                break;
            }
            case Op::FUSEUP:
                if (int rc = launch_fuse_up_op(fuse_ups[op.conv_idx], n, s)) return rc;
                ++launches;
                break;
            case Op::BILINEAR:
                if (dtype == 1) HIP_TRY(launch_bilinear2x_bf16(base(op.bin), base(op.bout), n, op.bin.c, op.bin.h, op.bin.w, s));
                else HIP_TRY(launch_bilinear2x(base(op.bin), base(op.bout), n, op.bin.c, op.bin.h, op.bin.w, s));
                ++launches;
                break;
            case Op::POOL:
                if (dtype == 1)
                    HIP_TRY(launch_softmax_pool_bf16(base(v_heat), v_heat.ctot, bf16_at(v_smpl_feats), 128, v_smpl_feats.ctot, bf16_at(v_csmap), 64,
                                                     v_csmap.ctot, d_stats, n, 56 * 56, s));
                else
                    HIP_TRY(launch_softmax_pool(base(v_heat), 25, base(v_smpl_feats), 128, base(v_csmap), 64, plf, csf, d_stats, n, 56 * 56, s));
                ++launches;
                break;
            case Op::TAIL:
                HIP_TRY(launch_head_tail(d_stats, true, plf, csf, tailw, rot6d, d_shape, d_cam, rotmat, theta, n, s));
                ++launches;
                break;
            case Op::SMPL:
                HIP_TRY(launch_smpl(d_shape, rotmat, d_cam, smpl, d_A, verts, kp3d, kp2d, n, s));
                launches += 4;
                break;
        }
        if (tl_end && !rec) HIP_TRY(hipEventRecord((*tl_end)[oi], s));
        if (lanes && op.record) HIP_TRY(hipEventRecord(op_events[oi], s));
        if (rec && !rec->deps.empty()) lane_last[lane] = op_node[oi] = rec->deps[0];
    }
    s = caller;
    if (lanes)
        for (int l = 1; l < lanes_used; ++l) {                // join: the caller's stream continues after every lane -- a lane whose last op lane 0 is
            if (!join_lane[l]) continue;                      // already behind through a kept wait needs no event
            HIP_TRY(hipEventRecord(ev_join[l], side[l]));
            HIP_TRY(hipStreamWaitEvent(s, ev_join[l], 0));
        }
    if (!convs_only) {
        auto copy_out = [&](float* dst, const float* src, size_t bytes) -> int {
            if (!dst) return 0;
            if (!rec) { HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s)); return 0; }
            std::vector<hipGraphNode_t> deps;
            for (hipGraphNode_t nd : lane_last) if (nd) deps.push_back(nd);
            hipGraphNode_t node = nullptr;
            HIP_TRY(hipGraphAddMemcpyNode1D(&node, rec->graph, deps.data(), deps.size(), dst, src, bytes, hipMemcpyDeviceToDevice));
            return 0;
        };
        int rc;
        if (dtype == 1) {                                   // the optional map outputs stay (N,C,56,56) fp32 for the caller
            auto conv_out = [&](float* dst, const View& v) -> int {
                if (!dst) return 0;
                if (rec) {
                    rec->deps.clear();
                    for (hipGraphNode_t nd : lane_last) if (nd) rec->deps.push_back(nd);
                }
                HIP_TRY(launch_nhwc_bf16_to_nchw_f32(base(v), dst, n, v.c, v.h, v.w, v.ctot, v.coff, s));
                return 0;
            };
            if ((rc = conv_out(o.features, v_cat))) return rc;
            if ((rc = conv_out(o.part_attn, v_heat))) return rc;
            if ((rc = conv_out(o.smpl_feats, v_smpl_feats))) return rc;
        } else {
        if ((rc = copy_out(o.features, base(v_cat), (size_t)n * 480 * 3136 * 4))) return rc;
        if ((rc = copy_out(o.part_attn, base(v_heat), (size_t)n * 25 * 3136 * 4))) return rc;
        if ((rc = copy_out(o.smpl_feats, base(v_smpl_feats), (size_t)n * 128 * 3136 * 4))) return rc;
        }
        launches_last = launches;
    }
    return 0;
}

// tail + SMPL from given pooled features; outputs as in enqueue() (NULL -> internal buffer)
int grnet::head_from_feats(const float* plf, const float* csf, int n, const grnet_outputs_t& o, hipStream_t s) {
    const auto [rot6d, rotmat, theta, verts, kp3d, kp2d] = head_outputs(o);
    HIP_TRY(launch_head_tail_from_feats(plf, csf, tailw, rot6d, d_shape, d_cam, rotmat, theta, n, s));
    HIP_TRY(launch_smpl(d_shape, rotmat, d_cam, smpl, d_A, verts, kp3d, kp2d, n, s));
    if (o.point_local_feat && o.point_local_feat != plf) HIP_TRY(hipMemcpyAsync(o.point_local_feat, plf, (size_t)n * 3072 * 4, hipMemcpyDeviceToDevice, s));
    if (o.cam_shape_feats && o.cam_shape_feats != csf) HIP_TRY(hipMemcpyAsync(o.cam_shape_feats, csf, (size_t)n * 1536 * 4, hipMemcpyDeviceToDevice, s));
    return 0;
}

// The use_gait_feat branch of GRNet.forward after the first head pass (grnet.py:154-173): cparams, FeatCorrector, second head pass,
// regressor.  plf (b*T,128,24), csf (b*T,64,24), cam (b*T rows of stride cam_ld: pred_cam, or theta with cam_ld = 85) are the first
// pass's results for the WHOLE clip(s); the second head pass runs in chunks of max_frames.
int grnet::gait_correct(const float* plf, const float* csf, const float* cam, int cam_ld, const float* bbox, const float* cimg, int b, int T,
                        const grnet_outputs_t& o, const grnet_gait_outputs_t& g, hipStream_t s) {
    if (int rc = gru_fault_check()) return rc;
    const size_t M = (size_t)b * T;
    const bool taps = taps_armed;
    if (taps) {
        size_t need = 0;
        if (featcorr_tap_floats(b, T, &need) != hipSuccess) { taps_armed = false; return fail(GRNET_EHIP, "device query for the tap layout failed"); }
        if (int rc = taps_begin(need + gru_tap_floats(b, T), "a gait-correction call")) return rc;
    }
    const size_t gru_need = gru_ws_floats(M, b);
    auto al = [](size_t f) { return (f + 63) & ~(size_t)63; };         // every sub-buffer starts 256-byte aligned (16-byte vector loads, 8-byte granules)
    const size_t own = al(M * 3) + al((size_t)b * 3) + al(M * 4) + al(M * 3072);
    float* ws = nullptr;
    if (int rc = temporal_scratch(kGemmWsFloats + gru_need + featcorr_ws_floats(b, T) + own, &ws)) return rc;
    GemmWorkspaceLease lease(ws, kGemmWsFloats);          // handed back on EVERY way out of this function
    float* p = ws + kGemmWsFloats;
    float* cparams = g.pred_cparam ? g.pred_cparam : p;   p += al(M * 3);
    float* avg = g.pred_avg ? g.pred_avg : p;             p += al((size_t)b * 3);
    float* phase = g.pred_phase ? g.pred_phase : p;       p += al(M * 4);
    float* new_plf = g.point_local_feat ? g.point_local_feat : p;   p += al(M * 3072);
    float* xc_buf = nullptr;
    const GruWorkspace w = gru_carve(p, M, b, &xc_buf);
    float* fws = p + gru_need;
    {
        TapLease tap_lease(taps ? &tap_sink : nullptr);   // the temporal launches only: the second head pass below is not tapped
        HIP_TRY(launch_gait_cparams(cam, cam_ld, bbox, cimg, cparams, (int)M, s));
        HIP_TRY(launch_gru(plf, cparams, gruw, w, avg, phase, xc_buf, b, T, s));
        HIP_TRY(launch_featcorr(plf, avg, phase, fcw, tsw, fws, new_plf, b, T, s));
    }
    for (size_t s0 = 0; s0 < M; s0 += (size_t)max_frames) {
        const int m = (int)std::min<size_t>((size_t)max_frames, M - s0);
        grnet_outputs_t oc{};
        oc.theta = o.theta ? o.theta + s0 * 85 : nullptr;
        oc.verts = o.verts ? o.verts + s0 * 6890 * 3 : nullptr;
        oc.kp_2d = o.kp_2d ? o.kp_2d + s0 * 58 : nullptr;
        oc.kp_3d = o.kp_3d ? o.kp_3d + s0 * 87 : nullptr;
        oc.rotmat = o.rotmat ? o.rotmat + s0 * 216 : nullptr;
        oc.pred_rot6d = o.pred_rot6d ? o.pred_rot6d + s0 * 144 : nullptr;
        if (int rc = head_from_feats(new_plf + s0 * 3072, csf + s0 * 1536, m, oc, s)) return rc;
    }
    return 0;
}

// Diagnostic: one eager forward on the lane streams with a timing event in front of and behind every op (after its cross-lane waits),
// un-traced -- rocprofv3's per-dispatch cost distorts a step of ~300 launches of 5-25 us.  Text: one line per op in enqueue order,
// "index lane start_us end_us label", times relative to the first op's start.  The events cost ~1 us of queue time each.
int grnet::op_timeline(const float* frames, int n, hipStream_t s, std::string& text) {
    if (!finalized) return fail(GRNET_ESTATE, "grnet_op_timeline before grnet_finalize_weights");
    if (!frames || n < 1 || n > max_frames) return fail(GRNET_EINVAL, "n_frames outside [1, max_frames]");
    if (!multi_lane) return fail(GRNET_ESTATE, "grnet_op_timeline needs GRNET_OPT_MULTI_LANE");
    const size_t m = ops_flat.size();
    std::vector<hipEvent_t> st(m, nullptr), en(m, nullptr);
    struct Cleanup {
        grnet* g; std::vector<hipEvent_t>*a, *b;
        ~Cleanup() { g->tl_start = g->tl_end = nullptr; for (auto e : *a) if (e) (void)hipEventDestroy(e); for (auto e : *b) if (e) (void)hipEventDestroy(e); }
    } cleanup{this, &st, &en};
    for (size_t i = 0; i < m; ++i) { HIP_TRY(hipEventCreate(&st[i])); HIP_TRY(hipEventCreate(&en[i])); }
    grnet_outputs_t o{};
    for (int rep = 0; rep < 3; ++rep) {                      // two warm passes, the third is reported
        tl_start = rep == 2 ? &st : nullptr;
        tl_end = rep == 2 ? &en : nullptr;
        int rc = enqueue(frames, n, o, s);
        tl_start = tl_end = nullptr;
        if (rc) return rc;
    }
    HIP_TRY(hipStreamSynchronize(s));
    text.clear();
    for (size_t i = 0; i < m; ++i) {
        float a = 0, b = 0;
        HIP_TRY(hipEventElapsedTime(&a, st[0], st[i]));
        HIP_TRY(hipEventElapsedTime(&b, st[0], en[i]));
        char line[400];
        snprintf(line, sizeof line, "%zu %d %.2f %.2f %s\n", i, ops_flat[i].lane, a * 1e3f, b * 1e3f, op_label(ops_flat[i]).c_str());
        text += line;
    }
    return 0;
}

// ------------------------------------------------------------------ tuning
// Measure, don't guess: time every launch configuration of every distinct convolution shape on this GPU
// for n frames (3 launches each, HIP events) and keep the fastest; then time whole forwards as a replayed hipGraph and as eager
// launches on the lane streams, with the cost model's and the measured table, and keep the fastest.  Activation buffers are used as
// scratch (contents are garbage afterwards, like after any forward).
int grnet::tune(int n, hipStream_t s, int level) {
    if (!finalized) return fail(GRNET_ESTATE, "grnet_tune before grnet_finalize_weights");
    if (n < 1 || n > max_frames) return fail(GRNET_EINVAL, "n_frames outside [1, max_frames]");
    static const int cands[] = {0, 14, 7, 1071, 1072, 1041, 1042, 1171, 1141};
    hipEvent_t e0 = nullptr, e1 = nullptr;
    // whatever way this function is left: events destroyed, half-built graphs dropped, the caller's schedule switches restored,
    // and -- unless the tuning completed -- no partial entry for n left behind
    struct Restore {
        grnet* g; int n; bool use_graph, done = false; hipEvent_t *e0, *e1;
        ~Restore() {
            if (*e0) (void)hipEventDestroy(*e0);
            if (*e1) (void)hipEventDestroy(*e1);
            g->drop_graphs();
            g->use_graph = use_graph;
            if (!done) { g->tuned_mode.erase(n); for (auto& L : g->convs) L.tuned.erase(n); }
        }
    } restore{this, n, use_graph, false, &e0, &e1};
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    std::map<std::tuple<int, int, int, int, int, int, int>, int> by_shape;
    for (auto& L : convs) {
        if (dtype == 1) { L.tuned[n] = 0; continue; }          // the bf16 kernel picks its tile by map width; only the schedule is timed
        const auto key = std::make_tuple(L.in.c, L.cout, L.ks, L.stride, L.in.h, (int)L.adds.size() + (L.solo ? 100 : 0), L.out.ctot);
        auto it = by_shape.find(key);
        if (it != by_shape.end()) { L.tuned[n] = it->second; continue; }
        float best = 1e30f, t_model = 1e30f;
        int best_hint = 0;
        for (int hint : cands) {
            ConvArgs a = conv_args(L, base(v_cat), n);        // any readable buffer stands in for the caller's frames
            if (launch_conv(a, s, hint) != hipSuccess) { (void)hipGetLastError(); continue; }
            HIP_TRY(hipEventRecord(e0, s));
            for (int r = 0; r < 3; ++r) (void)launch_conv(a, s, hint);
            HIP_TRY(hipEventRecord(e1, s));
            HIP_TRY(hipEventSynchronize(e1));
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
            if (hint == 0) t_model = ms;
            if (ms < best) { best = ms; best_hint = hint; }
        }
        // keep the cost model's choice unless a measured configuration is clearly (1.3x) faster in isolation:
        // close calls measured alone do not predict behaviour when several lanes share the CUs
        // (layers that run alone -- stem, layer1, PARE head -- take any measured gain above noise)
        if (!(t_model > (L.solo ? 1.06f : 1.3f) * best)) best_hint = 0;
        L.tuned[n] = best_hint;
        by_shape[key] = best_hint;
    }
    // schedule: {cost model, measured table} x {replayed hipGraph, eager launches on the four lane streams} -- the graph executor of
    // ROCm 7.2 maps parallel branches to fewer hardware queues than explicit streams do, so eager multi-stream launching can win
    // although it costs CPU time per launch.  Mode bits: 1 = measured per-shape table, 4 = eager.
    float t_mode[8];
    for (float& t : t_mode) t = 1e30f;
    const bool keep_graph = use_graph;
    for (int mode : {0, 1, 4, 5}) {
        if ((mode & 4) == 0 && !keep_graph) continue;                               // graphs not enabled by the caller
        if (dtype == 1 && (mode & 1)) continue;                                     // bf16: no per-shape table
        use_graph = (mode & 4) == 0;
        tuned_mode[n] = mode;
        drop_graphs();
        seen_once.clear();
        int rc = forward(base(v_cat), n, nullptr, s);          // first sight of the key: eager
        if (!rc) rc = forward(base(v_cat), n, nullptr, s);     // second: builds the graph, first replay
        if (rc) return rc;
        HIP_TRY(hipEventRecord(e0, s));
        for (int r = 0; r < 3; ++r) if ((rc = forward(base(v_cat), n, nullptr, s))) return rc;
        HIP_TRY(hipEventRecord(e1, s));
        HIP_TRY(hipEventSynchronize(e1));
        HIP_TRY(hipEventElapsedTime(&t_mode[mode], e0, e1));
    }
    use_graph = keep_graph;
    int best_mode = -1;
    for (int mode : {0, 1, 4, 5})
        if (t_mode[mode] < 1e30f && (best_mode < 0 || t_mode[mode] < t_mode[best_mode])) best_mode = mode;
    // three forwards per mode are a noisy clock (+-3 % from run to run on a shared node): a replayed graph has to win by more than that over the eager
    // launches of the same table to be taken (it never has: ROCm 7.2's executor deals the branches to fewer queues than the four lane streams)
    if (best_mode >= 0 && !(best_mode & 4) && t_mode[best_mode | 4] < 1e30f && t_mode[best_mode] > 0.97f * t_mode[best_mode | 4]) best_mode |= 4;
    if (best_mode < 0) return fail(GRNET_ESTATE, "no schedule could be timed");
    tuned_mode[n] = best_mode;
    // in-context refinement (level 2): greedy coordinate descent on the time of the whole replayed forward --
    // a configuration that wins alone can lose when four lanes share the CUs.  Shapes in order of their FLOP share.
    if (level >= 2) {
        use_graph = (best_mode & 4) == 0;
        tuned_mode[n] = best_mode | 1;                      // refine the measured table under the winning schedule
        auto time_forward = [&](float* out_ms) -> int {
            drop_graphs();
            seen_once.clear();
            int rc = forward(base(v_cat), n, nullptr, s);
            if (!rc) rc = forward(base(v_cat), n, nullptr, s);
            if (rc) return rc;
            float best_ms = 1e30f;
            for (int rep2 = 0; rep2 < 2; ++rep2) {
                HIP_TRY(hipEventRecord(e0, s));
                for (int r = 0; r < 2; ++r) if ((rc = forward(base(v_cat), n, nullptr, s))) return rc;
                HIP_TRY(hipEventRecord(e1, s));
                HIP_TRY(hipEventSynchronize(e1));
                float ms = 0;
                HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
                if (ms < best_ms) best_ms = ms;
            }
            *out_ms = best_ms / 2;
            return 0;
        };
        typedef std::tuple<int, int, int, int, int, int, int> Key;
        std::map<Key, double> share;
        auto key_of = [](const ConvLayer& L) { return std::make_tuple(L.in.c, L.cout, L.ks, L.stride, L.in.h, (int)L.adds.size(), L.out.ctot); };
        for (auto& L : convs) share[key_of(L)] += L.macs_per_frame;
        std::vector<std::pair<double, Key>> order;
        for (auto& kv : share) order.push_back({kv.second, kv.first});
        std::sort(order.begin(), order.end(), [](const std::pair<double, Key>& x, const std::pair<double, Key>& y) { return x.first > y.first; });
        float cur_ms = 0;
        int rc = time_forward(&cur_ms);
        if (rc) return rc;
        const float start_ms = cur_ms;
        for (auto& ok : order) {
            int keep_hint = 0;
            for (auto& L : convs) if (key_of(L) == ok.second) { keep_hint = L.tuned[n]; break; }
            int best_hint = keep_hint;
            for (int hint : cands) {
                if (hint == keep_hint) continue;
                bool valid = true;
                for (auto& L : convs)
                    if (key_of(L) == ok.second) {
                        ConvArgs a = conv_args(L, base(v_cat), n);
                        if (launch_conv(a, s, hint) != hipSuccess) { (void)hipGetLastError(); valid = false; }
                        break;
                    }
                if (!valid) continue;
                for (auto& L : convs) if (key_of(L) == ok.second) L.tuned[n] = hint;
                float ms = 0;
                if ((rc = time_forward(&ms))) return rc;
                if (ms < cur_ms * 0.995f) { cur_ms = ms; best_hint = hint; }
            }
            for (auto& L : convs) if (key_of(L) == ok.second) L.tuned[n] = best_hint;
        }
        if (getenv("GRNET_TRACE")) fprintf(stderr, "[grnet] in-context tuning n=%d: %.3f -> %.3f ms\n", n, start_ms, cur_ms);
        use_graph = keep_graph;
    }
    restore.done = true;
    seen_once.clear();
    if (getenv("GRNET_TRACE"))
        fprintf(stderr, "[grnet] tuned n=%d: forward ms graph[model %.3f measured %.3f] eager[model %.3f measured %.3f] -> mode %d\n",
                n, t_mode[0] / 3, t_mode[1] / 3, t_mode[4] / 3, t_mode[5] / 3, best_mode);
    return 0;
}

// ------------------------------------------------------------------ the forward and its graph cache
void grnet::drop_graphs() {
    for (auto& g : graphs) (void)hipGraphExecDestroy(g.second.exec);
    graphs.clear();
}

int grnet::forward(const float* frames, int n, const grnet_outputs_t* out, hipStream_t s) {
    if (!finalized) return fail(GRNET_ESTATE, "grnet_forward before grnet_finalize_weights");
    if (!frames || n < 1 || n > max_frames)
        return fail(GRNET_EINVAL, "n_frames " + std::to_string(n) + " outside [1, max_frames=" + std::to_string(max_frames) + "]");
    grnet_outputs_t o{};
    if (out) o = *out;
    last_n = n;
    {
        auto tm = tuned_mode.find(n);
        const bool eager_tuned = tm != tuned_mode.end() && (tm->second & 4);
        if (!use_graph || eager_tuned) return enqueue(frames, n, o, s);
    }
    GraphKey key{n, frames, o};
    auto it = graphs.find(key);
    // A caller that passes fresh output buffers every call (the Python shim does) rarely repeats a key, so a key is only
    // captured the SECOND time it is seen (first sight: eager launch, remembered in `seen_once`), and the cache keeps the
    // kMaxGraphs most recently used captured forwards: a steady-state key always ends up captured, one-off keys cost nothing.
    constexpr size_t kMaxGraphs = 16;
    if (it == graphs.end()) {
        bool seen = false;
        for (const GraphKey& k : seen_once) seen |= !(k < key) && !(key < k);
        if (!seen) {
            if (seen_once.size() >= 64) seen_once.erase(seen_once.begin());
            seen_once.push_back(key);
            return enqueue(frames, n, o, s);
        }
        if (graphs.size() >= kMaxGraphs) {
            auto lru = graphs.begin();
            for (auto g = graphs.begin(); g != graphs.end(); ++g)
                if (g->second.last_use < lru->second.last_use) lru = g;
            (void)hipGraphExecDestroy(lru->second.exec);
            graphs.erase(lru);
        }
    }
    if (it == graphs.end()) {
        hipGraph_t g = nullptr;
        HIP_TRY(hipGraphCreate(&g, 0));
        GraphRecorder recorder;
        recorder.graph = g;
        // GRNET_GRAPH_EDGES (diagnostic): 0 = dependencies given at node creation (edges in plan order; default), 1 = lane-chain edges first, 2 = cross-lane
        // edges first.  The order changes how ROCm 7.2's executor deals the nodes over its queues (108 / 26 / 142 / 16, 105 / 20 / 159 / 8, 116 / 90 / 70 / 16)
        // but none of them replays faster than 4.16 ms against 3.5 ms for the eager lane streams (profiles/r04_graph_vs_eager_timeline.txt)
        static const int edges_env = GRNET_AB(GRAPH_EDGES, 0);
        recorder.edge_order = edges_env;
        g_recorder = &recorder;
        int rc = enqueue(frames, n, o, s);
        g_recorder = nullptr;
        if (rc) { hipGraphDestroy(g); return rc; }
        hipError_t e = hipSuccess;
        if (recorder.edge_order) {
            auto add = [&](std::vector<hipGraphNode_t>& from, std::vector<hipGraphNode_t>& to) {
                if (e == hipSuccess && !from.empty()) e = hipGraphAddDependencies(g, from.data(), to.data(), from.size());
            };
            if (recorder.edge_order == 2) { add(recorder.cross_from, recorder.cross_to); add(recorder.chain_from, recorder.chain_to); }
            else { add(recorder.chain_from, recorder.chain_to); add(recorder.cross_from, recorder.cross_to); }
            if (e != hipSuccess) { hipGraphDestroy(g); return fail(GRNET_EHIP, std::string("hipGraphAddDependencies: ") + hipGetErrorString(e)); }
        }
        hipGraphExec_t ge = nullptr;
        e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
        hipGraphDestroy(g);
        if (e != hipSuccess) return fail(GRNET_EHIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
        it = graphs.emplace(key, GraphEntry{ge, 0}).first;
    }
    it->second.last_use = ++graph_clock;
    HIP_TRY(hipGraphLaunch(it->second.exec, s));
    return 0;
}
