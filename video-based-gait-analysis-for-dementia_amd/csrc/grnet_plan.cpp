// The network plan, the arena planner and the lane scheduler: everything about a forward that is decided without a device.  This file
// contains no HIP call -- grnet_arena_query / grnet_arena_layout run build_plan() and plan_arena() on a handle that never sees one.
//
// Topology restated from the reference constructors / forward passes (not translated from them):
//   backbone  lib/models/hrnet.py:469-536 with DOWNSAMPLE=False, USE_CONV=True (grnet.py:52-57)
//   head      lib/models/pare.py:245-303
//   regressor lib/models/pare.py:52-91, lib/models/smpl.py:149-191
// Data layout: fp32 NCHW, one buffer per intermediate tensor sized for max_frames images (the whole
// activation set is ~103 MB / frame, so 1 250 frames still fit the 288 GB of HBM3E); image stride is
// independent of the number of frames in a call, so a plan built once serves any n <= max_frames.  grnet_create_ex(GRNET_CREATE_COMPACT_ARENA)
// lets tensors whose lifetimes cannot overlap share memory instead (plan_arena: ~13.7 MB / frame, same launches, same bits).
#include "grnet_impl.h"
#include "lane_deps.h"

// ------------------------------------------------------------------ plan construction
View grnet::new_buffer(int c, int h, int w) {
    const int ct = dtype == 1 ? (c + 7) / 8 * 8 : c;     // NHWC bf16: 16-byte channel groups (the 25 heat channels -> 32)
    View v;
    v.slot = (int)buffer_floats.size();
    v.ctot = ct; v.coff = 0; v.c = c; v.h = h; v.w = w;
    buffer_floats.push_back((size_t)ct * h * w);
    return v;
}

View grnet::add_conv(View in, std::vector<ConvSeg> segs, int ks, int stride, bool relu, std::vector<AddRef> adds,
                     const View* out_override) {
    ConvLayer L;
    L.in = in;
    int cout = 0;
    for (auto& s : segs) cout += s.cout;
    const int pad = ks / 2;
    const int ho = (in.h + 2 * pad - ks) / stride + 1, wo = (in.w + 2 * pad - ks) / stride + 1;
    L.out = out_override ? *out_override : new_buffer(cout, ho, wo);
    L.segs = std::move(segs);
    L.cout = cout; L.ks = ks; L.stride = stride; L.relu = relu;
    L.adds = std::move(adds);
    L.cin_w = (dtype == 1 && in.c == 8 && in.ctot == 8) ? 3 : in.c;     // bf16 stem: 3 real channels stored as 8
    L.macs_per_frame = (double)ho * wo * cout * L.cin_w * ks * ks;
    L.lane_hint = cur_lane;
    L.solo = solo_region;
    convs.push_back(L);
    Op op;
    op.kind = Op::CONV;
    op.conv_idx = (int)convs.size() - 1;
    op.lane = cur_lane;
    ops.push_back(op);
    return convs.back().out;
}
View grnet::conv_bn(View in, const std::string& wkey, const std::string& bn, int cout, int ks, int stride, bool relu,
                    std::vector<AddRef> adds, const View* out_override) {
    return add_conv(in, {ConvSeg{wkey, bn, "", cout}}, ks, stride, relu, std::move(adds), out_override);
}

View grnet::add_bilinear(View in) {
    View out = new_buffer(in.c, in.h * 2, in.w * 2);
    Op op;
    op.kind = Op::BILINEAR;
    op.bin = in; op.bout = out;
    op.lane = cur_lane;
    ops.push_back(op);
    return out;
}

// HighResolutionModule (hrnet.py:249-267).  out0 (optional) receives fused output 0.
// Every branch convolution is its own launch on the lane of its branch; schedule_lanes() places the fuse layer's launches.
std::vector<View> grnet::hr_module(std::vector<View> xs, const std::string& p, const View* out0) {
    const int nb = (int)xs.size();
    std::vector<int> branch_tail(nb, -1);                               // plan index of the launch that writes x_b
    cur_lane = 0;
    std::vector<std::vector<int>> branch_ops(nb);                       // plan indices of the branch's convolutions, in order
    const std::string tag = p.substr(p.find("stage"));                  // "stage3.1."
    for (int k = 0; k < 4; ++k) {
        std::vector<View> y(nb);
        for (int b = 0; b < nb; ++b) {
            cur_lane = b;
            const std::string q = p + "branches." + std::to_string(b) + "." + std::to_string(k) + ".";
            y[b] = conv_bn(xs[b], q + "conv1.weight", q + "bn1", kBranchCh[b], 3, 1, true);
            name_view(tag + "b" + std::to_string(b) + "." + std::to_string(k) + ".conv1", y[b]);
            branch_ops[b].push_back((int)ops.size() - 1);
        }
        for (int b = 0; b < nb; ++b) {
            cur_lane = b;
            const std::string q = p + "branches." + std::to_string(b) + "." + std::to_string(k) + ".";
            xs[b] = conv_bn(y[b], q + "conv2.weight", q + "bn2", kBranchCh[b], 3, 1, true, {AddRef{xs[b], 0}});
            name_view(tag + "b" + std::to_string(b) + "." + std::to_string(k), xs[b]);
            branch_tail[b] = (int)ops.size() - 1;
            branch_ops[b].push_back((int)ops.size() - 1);
        }
    }
    // bf16: the branch's four BasicBlocks are also ONE chain launch (conv_bf16_chain.hip; taken in large calls, chain_active()).  The members
    // keep their own ops -- small calls launch them one by one -- and are pinned to one stream in order, so the events recorded behind the
    // (then empty) member ops still order every consumer behind the chain launch, which sits at the first member's place.
    if (dtype == 1)
        for (int b = 0; b < nb; ++b) {
            if (!conv_bf16_chain_eligible(kBranchCh[b], xs[b].w) || (int)branch_ops[b].size() > kMaxChain) continue;
            ChainPlan cp;
            cp.c = kBranchCh[b]; cp.w = xs[b].w;
            for (size_t i = 0; i < branch_ops[b].size(); ++i) {
                Op& op = ops[branch_ops[b][i]];
                convs[op.conv_idx].chain = (int)chains.size();
                convs[op.conv_idx].chain_pos = (int)i;
                cp.convs.push_back(op.conv_idx);
                if (i) op.follow = branch_ops[b][i - 1];
            }
            chains.push_back(cp);
        }
    for (int b = 0; b < nb; ++b) name_view(tag + "x" + std::to_string(b), xs[b]);
    // GRNET_FUSE_UP=0: the round-3 fuse layer (one 1x1 launch per up term, an elementwise launch for output 0)
    // (GRNET_BF16_FUSE_UP=0 does the same for the bf16 path, which has the grouped launch since round 5)
    static const int fuse_up_env = GRNET_AB(FUSE_UP, 1);
    const int fuse_up_bf_env = GRNET_AB(BF16_FUSE_UP, 0);    // read per handle: the tests build all three.  0 is the default: at 256 frames the lane-overlapped step is 10.68 / 10.91 / 10.67 ms for 0 / 1 / 2 (one lane: 11.69 / 11.39) -- the small launches hide behind the other lanes, the stored D_ij of layout 1 do not
    std::vector<View> outs = (dtype == 0 ? fuse_up_env : fuse_up_bf_env == 1) ? hr_fuse_grouped(xs, p, out0, branch_tail)
                                                                              : hr_fuse_separate(xs, p, out0, dtype == 1 && fuse_up_bf_env == 2, branch_tail);
    for (int i = 0; i < nb; ++i) name_view(tag + "y" + std::to_string(i), outs[i]);
    cur_lane = 0;
    return outs;
}

// Fuse layer, round 4 (hrnet.py:189-244 as used by :258-265).  Output i = relu(sum_j term_ij) with term_ij = x_i (j == i),
// nearest_up(BN(conv1x1(x_j))) (j > i), a chain of i-j stride-2 3x3 convolutions (j < i).  The branches of a module end at
// different times -- the 56x56 branch ~50 us before the 7x7 / 14x14 ones, which are the long pole of stages 3 and 4 -- so the
// layer is split by WHEN its inputs exist:
//   early: every down chain that starts at a branch b <= nb-3 runs to its end on that branch's own stream, right behind the
//          branch's last convolution (no cross-stream hop), as plain convolutions D_ij (no addend, no ReLU after the last one);
//          the first convolutions of the chains (i,0), i >= 2 (32 -> 32, ReLU) share their input and are one launch;
//   late:  ONE grouped launch (Op::FUSEUP, hr_fuse.hip) finishes outputs 0 .. nb-2 -- all 1x1 up terms, x_i, the D_ij, ReLU --
//          and ONE stride-2 convolution from branch nb-2 finishes output nb-1 (adds x_{nb-1} and the D_{nb-1,j}, ReLU).
// After the last branch output exists, every output of the module is ONE launch away (round 3: 1x1 launch -> sum / finishing
// convolution, up to four dependent launches with a cross-stream event between each pair).
// Stage 4: 8 launches per fuse layer (round 3: 17), stage 3: 4 (8), stage 2: 2 (3).
std::vector<View> grnet::hr_fuse_grouped(const std::vector<View>& xs, const std::string& p, const View* out0, const std::vector<int>& branch_tail) {
    const int nb = (int)xs.size();
    std::vector<View> outs(nb);
    auto key = [&](int i, int j, int level) { return p + "fuse_layers." + std::to_string(i) + "." + std::to_string(j) + "." + std::to_string(level) + "."; };
    std::vector<std::vector<View>> d(nb, std::vector<View>(nb));       // running tensor of chain (i,j)
    std::vector<std::vector<int>> d_op(nb, std::vector<int>(nb, -1));  // its latest launch
    for (int i = 1; i < nb; ++i)
        for (int j = 0; j < i; ++j) { d[i][j] = xs[j]; d_op[i][j] = branch_tail[j]; }
    auto follow_last = [&](int op_idx) { ops.back().follow = op_idx; };
    // every down-chain tensor is a tap of the fp32 plan, "<stage>.<m>.d<i>.<j>.<level>" (a merged first link: one name per slice)
    const std::string tag = p.substr(p.find("stage"));
    auto name_d = [&](int i, int j, int level) {
        if (dtype == 0) name_view(tag + "d" + std::to_string(i) + "." + std::to_string(j) + "." + std::to_string(level), d[i][j]);
    };
    // early: chains from branches 0 .. nb-3 (and, for outputs < nb-1, from branch nb-2 too: D_{i,i-1} with i <= nb-2 starts at a branch <= nb-3).
    // The first convolutions of all chains that start at one branch share their input and are ONE launch: the linear one ((j+1, j): the whole chain
    // of output j+1, no ReLU) first, then the ReLU'd first links of the longer chains (ConvLayer::relu_from)
    for (int j = 0; j < nb - 1; ++j)
        for (int level = 0; level < nb - 1 - j; ++level) {
            std::vector<int> members;                                   // outputs i whose chain (i, j) has a convolution at this level
            for (int i = j + 1; i < nb; ++i)
                if (level < i - j && !(i == nb - 1 && j == nb - 2)) members.push_back(i);
            // GRNET_FUSE_MERGE (A/B switch): 2 = all first convolutions of a branch in one launch, 1 = only the ReLU'd ones, 0 = none
            // (the bf16 kernels have no per-segment ReLU: every first convolution is its own launch there)
            static const int merge_env_f32 = GRNET_AB(FUSE_MERGE, 2);
            const int merge_env = dtype == 1 ? 0 : merge_env_f32;
            std::vector<int> solo;
            if (level == 0 && merge_env < 2) {
                std::vector<int> keep;
                for (int i : members) (merge_env == 1 && i - j >= 2 ? keep : solo).push_back(i);
                members.swap(keep);
            }
            if (level == 0 && members.size() >= 2) {
                std::vector<ConvSeg> segs;
                int lin = 0;
                for (int i : members) {
                    const bool last = i - j == 1;
                    segs.push_back(ConvSeg{key(i, j, 0) + "0.weight", key(i, j, 0) + "1", "", last ? kBranchCh[i] : kBranchCh[j]});
                    if (last) lin += kBranchCh[i];
                }
                cur_lane = j;
                View m = add_conv(xs[j], segs, 3, 2, true);
                convs.back().relu_from = lin;                            // members are in ascending i: the linear segment (i = j + 1), if any, comes first
                follow_last(branch_tail[j]);
                int off = 0;
                for (int i : members) {
                    const int c = i - j == 1 ? kBranchCh[i] : kBranchCh[j];
                    d[i][j] = slice(m, off, c);
                    d_op[i][j] = (int)ops.size() - 1;
                    off += c;
                    name_d(i, j, 0);
                }
                members.clear();
            }
            members.insert(members.begin(), solo.begin(), solo.end());
            for (int i : members) {
                const bool last = level == i - j - 1;
                cur_lane = j;
                d[i][j] = conv_bn(d[i][j], key(i, j, level) + "0.weight", key(i, j, level) + "1", last ? kBranchCh[i] : kBranchCh[j], 3, 2, !last);
                follow_last(d_op[i][j]);
                d_op[i][j] = (int)ops.size() - 1;
                name_d(i, j, level);
            }
        }
    // late: the grouped launch for outputs 0 .. nb-2 ...
    FuseUpPlan fp;
    fp.nb = nb; fp.prefix = p; fp.xs = xs;
    for (int i = 0; i < nb - 1; ++i) {
        outs[i] = (i == 0 && out0) ? *out0 : new_buffer(kBranchCh[i], xs[i].h, xs[i].w);
        fp.outs.push_back(outs[i]);
        fp.extra.push_back({});
        for (int j = 0; j < i; ++j) fp.extra.back().push_back(d[i][j]);
    }
    for (int i = 0; i < nb - 1; ++i)
        for (int j = i + 1; j < nb; ++j) fp.macs_per_frame += (double)xs[j].h * xs[j].w * kBranchCh[j] * kBranchCh[i];
    fuse_ups.push_back(fp);
    Op op;
    op.kind = Op::FUSEUP;
    op.conv_idx = (int)fuse_ups.size() - 1;
    op.lane = cur_lane = nb - 1;
    op.follow = branch_tail[nb - 1];
    ops.push_back(op);
    // ... and the stride-2 convolution from branch nb-2 that finishes output nb-1
    {
        const int i = nb - 1;
        std::vector<AddRef> adds;
        adds.push_back(AddRef{xs[i], 0});
        for (int j = 0; j < i - 1; ++j) adds.push_back(AddRef{d[i][j], 0});
        cur_lane = nb - 2;
        outs[i] = conv_bn(xs[i - 1], key(i, i - 1, 0) + "0.weight", key(i, i - 1, 0) + "1", kBranchCh[i], 3, 2, true, adds);
        follow_last(branch_tail[i - 1]);
    }
    return outs;
}
// the convolutions added last (in order) become ONE row-walking launch in large bf16 calls; the members keep their own ops (small calls launch them one by
// one), pinned to the launcher's stream in order -- the mechanism of the BasicBlock chains
void grnet::add_roll(int kind, int n_convs) {
    RollPlan rp;
    rp.kind = kind;
    const int first = (int)convs.size() - n_convs;
    for (int i = 0; i < n_convs; ++i) {
        convs[first + i].roll = (int)rolls.size();
        convs[first + i].roll_pos = i;
        rp.convs.push_back(first + i);
    }
    int prev_op = -1;
    for (int i = 0; i < (int)ops.size(); ++i)
        if (ops[i].kind == Op::CONV && ops[i].conv_idx >= first) {
            if (prev_op >= 0) ops[i].follow = prev_op;
            prev_op = i;
        }
    rolls.push_back(rp);
}

// Fuse layer as launched until round 3 (kept for the bf16 path and for A/B runs)
// up0 (bf16, round 5): output 0 -- the full-resolution one, 4 of the layer's launches -- is finished by ONE hr_fuse_up_bf16 launch instead (only = 0);
// the other outputs keep their finishing stride-2 convolution, which adds everything in its epilogue and writes no D_ij to memory
std::vector<View> grnet::hr_fuse_separate(std::vector<View> xs, const std::string& p, const View* out0, bool up0, const std::vector<int>& branch_tail) {
    const int nb = (int)xs.size();
    // up terms t[i][j], j > i: conv1x1 + BN at the resolution of branch j (nearest upsample is
    // applied where the term is consumed: it commutes with the per-pixel conv/BN)
    std::vector<std::vector<View>> t(nb, std::vector<View>(nb));
    // the up terms W_ij x_j of ONE source branch j (linear 1x1 convolutions at the source's resolution) share their input: one launch, output channels side by side
    // (round 5; 31 -> 18 launches of the 1x1 terms per forward, 10.28 against 10.34 ms at 256 frames bf16; GRNET_FUSE_MERGE_UP=0: one launch per term)
    static const int merge_up_env = GRNET_AB(FUSE_MERGE_UP, 1);
    std::vector<std::vector<char>> tdone(nb, std::vector<char>(nb, 0));
    if (merge_up_env)
        for (int j = 1; j < nb; ++j) {
            std::vector<int> members;
            for (int i = (up0 ? 1 : 0); i < j; ++i) members.push_back(i);
            if (members.size() < 2) continue;
            std::vector<ConvSeg> segs;
            for (int i : members) {
                const std::string q = p + "fuse_layers." + std::to_string(i) + "." + std::to_string(j) + ".";
                segs.push_back(ConvSeg{q + "0.weight", q + "1", "", kBranchCh[i]});
            }
            cur_lane = j;
            View m = add_conv(xs[j], segs, 1, 1, false);
            int off = 0;
            for (int i : members) { t[i][j] = slice(m, off, kBranchCh[i]); off += kBranchCh[i]; tdone[i][j] = 1; }
        }
    for (int i = 0; i < nb; ++i)
        for (int j = i + 1; j < nb; ++j) {
            if (up0 && i == 0) continue;
            if (tdone[i][j]) continue;
            const std::string q = p + "fuse_layers." + std::to_string(i) + "." + std::to_string(j) + ".";
            cur_lane = j;
            t[i][j] = conv_bn(xs[j], q + "0.weight", q + "1", kBranchCh[i], 1, 1, false);
        }
    cur_lane = 0;
    std::vector<View> outs(nb);
    if (up0) {
        FuseUpPlan fp;
        fp.nb = nb; fp.prefix = p; fp.xs = xs; fp.only = 0;
        outs[0] = out0 ? *out0 : new_buffer(kBranchCh[0], xs[0].h, xs[0].w);
        fp.outs.push_back(outs[0]);
        fp.extra.push_back({});
        for (int j = 1; j < nb; ++j) fp.macs_per_frame += (double)xs[j].h * xs[j].w * kBranchCh[j] * kBranchCh[0];
        fuse_ups.push_back(fp);
        Op op;
        op.kind = Op::FUSEUP;
        op.conv_idx = (int)fuse_ups.size() - 1;
        op.lane = 0;
        op.follow = branch_tail[0];
        ops.push_back(op);
    } else {   // output 0: elementwise sum of the identity and the upsampled terms
        View o = out0 ? *out0 : new_buffer(kBranchCh[0], xs[0].h, xs[0].w);
        Op op;
        op.kind = Op::SUM;
        op.lane = 0;
        SumArgs& sa = op.sum;
        sa.C = kBranchCh[0]; sa.H = xs[0].h; sa.W = xs[0].w; sa.relu = 1;
        sa.n_add = nb;
        sum_views.push_back({o, {}});
        sum_views.back().adds.push_back(AddRef{xs[0], 0});
        for (int j = 1; j < nb; ++j) sum_views.back().adds.push_back(AddRef{t[0][j], j});
        op.conv_idx = (int)sum_views.size() - 1;
        ops.push_back(op);
        outs[0] = o;
    }
    // down paths (all 3x3 stride 2), by dependency level: chain conv k of (i,j) is level k; the conv that
    // finishes output i (the single stride-2 conv from branch i-1, which also adds the identity, the
    // finished down chains and the upsampled terms, then applies the ReLU) is level 0 for i = 1, else i.
    std::vector<std::vector<View>> d(nb, std::vector<View>(nb));       // running tensor of chain (i,j)
    for (int i = 2; i < nb; ++i)
        for (int j = 0; j < i - 1; ++j) d[i][j] = xs[j];
    for (int level = 0; level < nb; ++level) {
        // the ReLU'd first links of the chains that start at ONE branch share their input: one launch with their output channels side by side (round 5, bf16 as well:
        // stage 4's chains (2,0) and (3,0) read the 56x56 branch once instead of twice).  GRNET_FUSE_MERGE_FIRST=0: one launch per chain
        static const int merge_first_env = GRNET_AB(FUSE_MERGE_FIRST, 1);
        std::vector<std::vector<char>> merged(nb, std::vector<char>(nb, 0));
        if (level == 0 && merge_first_env)
            for (int j = 0; j < nb - 2; ++j) {
                std::vector<int> members;
                for (int i = j + 2; i < nb; ++i)
                    if (i - j - 1 > 0) members.push_back(i);                   // chain (i, j) has more than one link: its first link is ReLU'd, kBranchCh[j] channels
                if (members.size() < 2) continue;
                std::vector<ConvSeg> segs;
                for (int i : members) {
                    const std::string q = p + "fuse_layers." + std::to_string(i) + "." + std::to_string(j) + ".0.";
                    segs.push_back(ConvSeg{q + "0.weight", q + "1", "", kBranchCh[j]});
                }
                cur_lane = j;
                View m = add_conv(xs[j], segs, 3, 2, true);
                int off = 0;
                for (int i : members) { d[i][j] = slice(m, off, kBranchCh[j]); off += kBranchCh[j]; merged[i][j] = 1; }
            }
        for (int i = 2; i < nb; ++i)
            for (int j = 0; j < i - 1; ++j) {
                if (level >= i - j) continue;
                if (merged[i][j]) continue;
                const bool last = level == i - j - 1;
                cur_lane = j;
                const std::string q = p + "fuse_layers." + std::to_string(i) + "." + std::to_string(j) + "." + std::to_string(level) + ".";
                d[i][j] = conv_bn(d[i][j], q + "0.weight", q + "1", last ? kBranchCh[i] : kBranchCh[j], 3, 2, !last);
            }
        for (int i = 1; i < nb; ++i) {
            if ((i == 1 ? 0 : i) != level) continue;
            std::vector<AddRef> adds;
            adds.push_back(AddRef{xs[i], 0});
            for (int j = 0; j < i - 1; ++j) adds.push_back(AddRef{d[i][j], 0});
            for (int j = i + 1; j < nb; ++j) adds.push_back(AddRef{t[i][j], j - i});
            cur_lane = i;
            const std::string q = p + "fuse_layers." + std::to_string(i) + "." + std::to_string(i - 1) + ".0.";
            outs[i] = conv_bn(xs[i - 1], q + "0.weight", q + "1", kBranchCh[i], 3, 2, true, adds);
        }
    }
    cur_lane = 0;
    return outs;
}

void grnet::build_plan() {
    const std::string b = "backbone.";
    v_input.ctot = 3; v_input.coff = 0; v_input.c = 3; v_input.h = 224; v_input.w = 224;
    View in = v_input;
    in.slot = View::kFrames;
    // bf16: the stem's first convolution reads the caller's fp32 frames itself (conv_bf16_stem, round 4); GRNET_BF16_STEM=0 restores the
    // conversion launch -- frames (N,3,224,224) f32 -> NHWC bf16, 8 channels per pixel -- in front of the generic kernel
    static const int bf16_stem_env = GRNET_AB(BF16_STEM, 1);
    bf16_stem = dtype == 1 && bf16_stem_env;
    if (dtype == 1 && !bf16_stem) {
        v_in8 = new_buffer(8, 224, 224);
        Op cv;
        cv.kind = Op::CONVERT;
        ops.push_back(cv);
        in = v_in8;
    }
    solo_region = true;
    View x = conv_bn(in, b + "conv1.weight", b + "bn1", 64, 3, 2, true);
    name_view("stem_conv1", x);
    x = conv_bn(x, b + "conv2.weight", b + "bn2", 64, 3, 2, true);
    name_view("stem_conv2", x);
    if (bf16_stem) add_roll(0, 2);
    int prev_conv3 = -1;
    for (int k = 0; k < 4; ++k) {                       // layer1: 4 Bottlenecks (hrnet.py:80-100)
        const std::string q = b + "layer1." + std::to_string(k) + ".";
        // bf16: Bottleneck k-1's expansion and this one's reduction are a PAIR (one launch in large calls): the reduction is the first convolution added below
        const int first_new = (int)convs.size() + ((k == 0 && !(dtype == 1 && (GRNET_AB(BF16_MERGE_DS, 1)))) ? 1 : 0);
        struct PairAtExit {
            grnet* g; int& prev; int first_new;
            ~PairAtExit() {
                if (g->dtype == 1 && prev >= 0 && first_new < (int)g->convs.size() && g->convs[first_new].ks == 1 && g->convs[first_new].in.c == 256 && g->convs[first_new].cout == 64) {
                    g->convs[prev].pair_next = first_new;
                    g->convs[first_new].pair_of = prev;
                    int op_prev = -1, op_new = -1;                 // the member launches nothing in large calls: it shares the expansion's stream, so that a graph
                    for (int i = 0; i < (int)g->ops.size(); ++i) {  // recorded from this plan hangs the member's consumers on the expansion's node (round-5 advice)
                        if (g->ops[i].kind == Op::CONV && g->ops[i].conv_idx == prev) op_prev = i;
                        if (g->ops[i].kind == Op::CONV && g->ops[i].conv_idx == first_new) op_new = i;
                    }
                    if (op_prev >= 0 && op_new >= 0) g->ops[op_new].follow = op_prev;
                }
                prev = (int)g->convs.size() - 1;         // this Bottleneck's conv3 is the last convolution added
            }
        } pair_at_exit{this, prev_conv3, first_new};
        // bf16, first Bottleneck: relu(BN3(conv3(t)) + BNd(downsample(x))) is ONE 1x1 GEMM over the concatenated inputs [t ; x] (K = 64 + 64, the two
        // BatchNorms folded into their halves of the weights, the shifts summed): the 411 MB downsample tensor (at 256 frames) is neither written nor read
        // back, and a launch goes away.  GRNET_BF16_MERGE_DS=0: the two launches of the reference's graph (hrnet.py:80-100, 389-406).
        static const int merge_ds = GRNET_AB(BF16_MERGE_DS, 1);
        const std::string tq = "layer1." + std::to_string(k) + ".";
        if (k == 0 && dtype == 1 && merge_ds) {
            View y = conv_bn(x, q + "conv1.weight", q + "bn1", 64, 1, 1, true);
            name_view(tq + "conv1", y);
            y = conv_bn(y, q + "conv2.weight", q + "bn2", 64, 3, 1, true);
            name_view(tq + "conv2", y);
            View xin = x;
            x = conv_bn(y, q + "conv3.weight", q + "bn3", 256, 1, 1, true);
            convs.back().in2 = xin;
            convs.back().seg2 = ConvSeg{q + "downsample.0.weight", q + "downsample.1", "", 256};
            convs.back().macs_per_frame *= 2;                  // K = 64 (t) + 64 (x)
            add_roll(1, 3);
            name_view("layer1.0", x);
            continue;
        }
        View res = k == 0 ? conv_bn(x, q + "downsample.0.weight", q + "downsample.1", 256, 1, 1, false) : x;
        if (k == 0) name_view(tq + "downsample", res);
        View y = conv_bn(x, q + "conv1.weight", q + "bn1", 64, 1, 1, true);
        name_view(tq + "conv1", y);
        y = conv_bn(y, q + "conv2.weight", q + "bn2", 64, 3, 1, true);
        name_view(tq + "conv2", y);
        x = conv_bn(y, q + "conv3.weight", q + "bn3", 256, 1, 1, true, {AddRef{res, 0}});
        if (dtype == 1 && k > 0) add_roll(2, 3);
        name_view("layer1." + std::to_string(k), x);
    }
    name_view("layer1", x);
    solo_region = false;
    std::vector<View> xs;
    xs.push_back(conv_bn(x, b + "transition1.0.0.weight", b + "transition1.0.1", 32, 3, 1, true));
    name_view("transition1.0", xs.back());
    cur_lane = 1;
    xs.push_back(conv_bn(x, b + "transition1.1.0.0.weight", b + "transition1.1.0.1", 64, 3, 2, true));
    name_view("transition1.1", xs.back());
    cur_lane = 0;
    xs = hr_module(xs, b + "stage2.0.", nullptr);
    for (size_t i = 0; i < xs.size(); ++i) name_view("stage2." + std::to_string(i), xs[i]);
    cur_lane = 2;
    xs.push_back(conv_bn(xs.back(), b + "transition2.2.0.0.weight", b + "transition2.2.0.1", 128, 3, 2, true));
    name_view("transition2.2", xs.back());
    cur_lane = 0;
    for (int m = 0; m < 4; ++m) xs = hr_module(xs, b + "stage3." + std::to_string(m) + ".", nullptr);
    for (size_t i = 0; i < xs.size(); ++i) name_view("stage3." + std::to_string(i), xs[i]);
    cur_lane = 3;
    xs.push_back(conv_bn(xs.back(), b + "transition3.3.0.0.weight", b + "transition3.3.0.1", 256, 3, 2, true));
    name_view("transition3.3", xs.back());
    cur_lane = 0;
    v_cat = new_buffer(480, 56, 56);                    // torch.cat([x0, x1, x2, x3], 1) (hrnet.py:524)
    name_view("cat", v_cat);
    for (int m = 0; m < 3; ++m) {
        View o0 = slice(v_cat, 0, 32);
        xs = hr_module(xs, b + "stage4." + std::to_string(m) + ".", m == 2 ? &o0 : nullptr);
    }
    for (size_t i = 0; i < xs.size(); ++i) name_view("stage4." + std::to_string(i), xs[i]);
    int coff = 32;
    for (int idx = 2; idx <= 4; ++idx) {                // upsample heads (hrnet.py:440-453,521-523)
        const int br = idx - 1, c = kBranchCh[br], n_layers = idx - 1;
        cur_lane = br;                                  // the three upsample heads are independent
        View t = xs[br];
        for (int l = 0; l < n_layers; ++l) {
            const std::string q = b + "upsample_stage_" + std::to_string(idx) + ".";
            View up = add_bilinear(t);
            name_view("up" + std::to_string(idx) + "." + std::to_string(l) + ".bilinear", up);
            View dst = slice(v_cat, coff, c);
            t = conv_bn(up, q + std::to_string(4 * l + 1) + ".weight", q + std::to_string(4 * l + 2), c, 3, 1, true, {},
                        l == n_layers - 1 ? &dst : nullptr);
            name_view("up" + std::to_string(idx) + "." + std::to_string(l) + ".conv", t);
        }
        coff += c;
    }
    cur_lane = 0;
    // PARE head (pare.py:305-336).  The two 480->128 first convolutions read the same input and are
    // issued as one 480->256 convolution writing both halves of one buffer.
    const std::string hd = "head.";
    solo_region = true;
    View first = add_conv(v_cat,
                          {ConvSeg{hd + "keypoint_deconv_layers.0.weight", hd + "keypoint_deconv_layers.1", "", 128},
                           ConvSeg{hd + "smpl_deconv_layers.0.weight", hd + "smpl_deconv_layers.1", "", 128}},
                          3, 1, true);
    name_view("head.first", first);
    View part_feats = conv_bn(slice(first, 0, 128), hd + "keypoint_deconv_layers.3.weight", hd + "keypoint_deconv_layers.4", 128, 3, 1, true);
    name_view("head.part_feats", part_feats);
    v_heat = add_conv(part_feats, {ConvSeg{hd + "keypoint_final_layer.weight", "", hd + "keypoint_final_layer.bias", 25}}, 1, 1, false);
    name_view("head.heat", v_heat);
    cur_lane = 1;                                       // the 3D branch runs beside the 2D branch
    v_smpl_feats = conv_bn(slice(first, 128, 128), hd + "smpl_deconv_layers.3.weight", hd + "smpl_deconv_layers.4", 128, 3, 1, true);
    name_view("head.smpl_feats", v_smpl_feats);
    v_csmap = add_conv(v_smpl_feats, {ConvSeg{hd + "smpl_final_layer.weight", "", hd + "smpl_final_layer.bias", 64}}, 1, 1, false);
    name_view("head.cam_shape", v_csmap);
    cur_lane = 0;
    solo_region = false;
    Op op;
    op.kind = Op::POOL; ops.push_back(op);
    op.kind = Op::TAIL; ops.push_back(op);
    op.kind = Op::SMPL; ops.push_back(op);
    annotate_plan();
}

// Read-after-write edges between lanes.  Every op writes a tensor nobody has written before (the writers of the concat buffer own
// disjoint channel slices), so RAW edges are the only hazards the schedule has to order inside one forward; forwards are separated by
// the join at the end of enqueue().  A tensor is a planned buffer (slot), not an address and not a view: in a compact arena
// (GRNET_CREATE_COMPACT_ARENA) several tensors live at one address, and the sharing rule of plan_arena() makes the RAW edges computed
// here order them as well -- a compact handle gets exactly the edges, lanes and events of a full one.
// Slots an op reads / writes (the caller's frames are no planned buffer: dropped).
void grnet::op_reads(const Op& op, std::vector<int>& r) const {
    r.clear();
    auto put = [&](const View& v) { if (v.slot >= 0) r.push_back(v.slot); };
    switch (op.kind) {
        case Op::CONV: {
            const ConvLayer& L = convs[op.conv_idx];
            put(L.in);
            if (L.in2.c) put(L.in2);
            for (auto& a : L.adds) put(a.v);
            break;
        }
        case Op::SUM:
            for (auto& a : sum_views[op.conv_idx].adds) put(a.v);
            break;
        case Op::BILINEAR: put(op.bin); break;
        case Op::FUSEUP:
        {
            const FuseUpPlan& fp = fuse_ups[op.conv_idx];
            for (size_t j = fp.only < 0 ? 0 : fp.only; j < fp.xs.size(); ++j) put(fp.xs[j]);
            for (size_t i = 0; i < fp.extra.size(); ++i)
                if (fp.only < 0 || fp.only == (int)i) for (auto& v : fp.extra[i]) put(v);
        }
            break;
        case Op::POOL: put(v_heat); put(v_smpl_feats); put(v_csmap); break;
        default: break;                                     // TAIL / SMPL follow POOL on lane 0
    }
}
void grnet::op_writes(const Op& op, std::vector<int>& w) const {
    w.clear();
    auto put = [&](const View& v) { if (v.slot >= 0) w.push_back(v.slot); };
    if (op.kind == Op::CONV) put(convs[op.conv_idx].out);
    else if (op.kind == Op::SUM) put(sum_views[op.conv_idx].out);
    else if (op.kind == Op::BILINEAR) put(op.bout);
    else if (op.kind == Op::CONVERT) put(v_in8);
    else if (op.kind == Op::FUSEUP) {
        const FuseUpPlan& fp = fuse_ups[op.conv_idx];
        for (size_t i = 0; i < fp.outs.size(); ++i) if (fp.only < 0 || fp.only == (int)i) put(fp.outs[i]);
    }
}
// End of build_plan(): what the lane scheduler and the arena planner read.
void grnet::annotate_plan() {
    for (Op& op : ops) { op_reads(op, op.rd); op_writes(op, op.wr); }
    end_reads = {v_cat.slot, v_heat.slot, v_smpl_feats.slot};
}

std::string grnet::op_label(const Op& op) const {
    switch (op.kind) {
        case Op::CONV: {
            const ConvLayer& L = convs[op.conv_idx];
            char b[256];
            snprintf(b, sizeof b, "conv %dx%d s%d %d->%d @%d %s", L.ks, L.ks, L.stride, L.in.c, L.cout, L.in.w, L.segs.empty() ? "" : L.segs[0].wkey.c_str());
            return b;
        }
        case Op::FUSEUP: return "fuse_up " + fuse_ups[op.conv_idx].prefix;
        case Op::SUM: return "fuse_sum";
        case Op::BILINEAR: return "bilinear2x c" + std::to_string(op.bin.c) + " @" + std::to_string(op.bin.w);
        case Op::POOL: return "attn_pool";
        case Op::TAIL: return "head_tail";
        case Op::SMPL: return "smpl";
        case Op::CONVERT: return "convert";
    }
    return "?";
}

// ------------------------------------------------------------------ the activation arena
// Full layout (the default): every tensor has its own bytes, so every intermediate of a forward can be read afterwards (grnet_debug_tensor).
// Compact layout (GRNET_CREATE_COMPACT_ARENA): tensors whose lifetimes cannot overlap share bytes.  THE RULE: A may lie under B only if every op
// that reads or writes A is a strict ancestor, in the read-after-write DAG of the plan, of every op that writes B.  Nothing is added to make that
// true -- no edge, no event, no wait: FIFO streams and the events analyze_dependencies() places anyway enforce ancestor order for any lane
// schedule, so the launches, the schedule, the captured graph and the outputs of a compact handle are those of a full one.  Strictness keeps an
// op's output off its own inputs.
// The rule has to hold for every launch form the plan can take (any call size, any tuning table, any GRNET_OPT_BF16_CHAIN mask).  The bf16 kernel
// groups run several member ops as ONE launch (BasicBlock chains, row walkers, the layer1 expansion + reduction pair): that launch reads the
// group's inputs for as long as it writes the group's outputs, although in the un-grouped DAG a chain's input is dead before the chain's last
// convolution writes.  So every tensor a group member writes also conflicts with every tensor any member touches -- which is the rule again on
// the DAG with the group contracted to one node -- and the conflict relation is the union over the un-grouped form and every group.
// (The fp32 fuse launch is ONE op that reads and writes what all its per-output forms together would: FuseUpPlan::only < 0 in op_reads.)
// Tensors the forward's copy-outs read after the op list (end_reads) are touched by a virtual last op: nothing is ever placed over them.

// Op indices (plan order) that some launch form runs as ONE launch: the bf16 chains, row walkers and layer1 pairs
std::vector<std::vector<int>> grnet::launch_groups() const {
    std::vector<std::vector<int>> g;
    std::vector<int> op_of(convs.size(), -1);
    for (int i = 0; i < (int)ops.size(); ++i)
        if (ops[i].kind == Op::CONV) op_of[ops[i].conv_idx] = i;
    auto add = [&](const std::vector<int>& cv) {
        std::vector<int> m;
        for (int c : cv) if (op_of[c] >= 0) m.push_back(op_of[c]);
        std::sort(m.begin(), m.end());
        if (m.size() >= 2) g.push_back(m);
    };
    for (const ChainPlan& c : chains) add(c.convs);
    for (const RollPlan& r : rolls) add(r.convs);
    for (int i = 0; i < (int)convs.size(); ++i)
        if (convs[i].pair_next >= 0) add({i, convs[i].pair_next});
    return g;
}

namespace grnet_detail {
// Offsets for n buffers of which some pairs may not overlap (grnet_arena_assign): largest first (ties: lowest index), each at the lowest
// aligned offset where it overlaps no conflicting buffer placed before it.  A deterministic function of (sizes, conflicts).  Sizes, offsets
// and the total are in one unit (bytes at the ABI, floats inside the library); `align` is in that unit.
void arena_first_fit(const std::vector<int64_t>& sizes, const std::vector<std::vector<int>>& adj, int64_t align, std::vector<int64_t>& off, int64_t* total) {
    const int n = (int)sizes.size();
    std::vector<int64_t> sz(n);
    for (int i = 0; i < n; ++i) sz[i] = (sizes[i] + align - 1) / align * align;
    std::vector<int> order(n);
    for (int i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return sz[a] > sz[b]; });
    off.assign(n, 0);
    std::vector<char> placed(n, 0);
    std::vector<std::pair<int64_t, int64_t>> busy;
    int64_t end = 0;
    for (int t : order) {
        busy.clear();
        for (int u : adj[t])
            if (placed[u] && sz[u] > 0) busy.emplace_back(off[u], off[u] + sz[u]);
        std::sort(busy.begin(), busy.end());
        int64_t cur = 0;
        for (auto& iv : busy) {
            if (cur + sz[t] <= iv.first) break;
            cur = std::max(cur, iv.second);
        }
        off[t] = cur;
        placed[t] = 1;
        end = std::max(end, cur + sz[t]);
    }
    *total = end;
}
}  // namespace grnet_detail

// Host code only (no HIP call): grnet_arena_query / grnet_arena_layout run it on a plan that never sees a device.
int grnet::plan_arena(bool compact_layout, ArenaPlan& ap) const {
    const int nt = (int)buffer_floats.size(), m = (int)ops.size() + 1;      // + the virtual copy-out op
    ap = ArenaPlan();
    ap.floats.resize(nt);
    for (int t = 0; t < nt; ++t) ap.floats[t] = ((int64_t)buffer_floats[t] * max_frames + kArenaAlign - 1) / kArenaAlign * kArenaAlign;
    ap.rd.resize(m); ap.wr.resize(m);
    for (int i = 0; i + 1 < m; ++i) { ap.rd[i] = ops[i].rd; ap.wr[i] = ops[i].wr; }
    for (int s : end_reads) if (s >= 0) ap.rd[m - 1].push_back(s);
    ap.groups = launch_groups();
    // strict ancestors over the RAW edges, as analyze_dependencies() derives them (plan order is a topological order)
    const int words = (m + 63) / 64;
    std::vector<std::vector<uint64_t>> anc(m, std::vector<uint64_t>(words, 0));
    auto is_anc = [&](int a, int of) { return (anc[of][a >> 6] >> (a & 63)) & 1; };
    std::vector<std::vector<int>> writers(nt), touch(nt);
    for (int i = 0; i < m; ++i) {
        for (int t : ap.rd[i])
            for (int w : writers[t]) {
                for (int k = 0; k < words; ++k) anc[i][k] |= anc[w][k];
                anc[i][w >> 6] |= 1ull << (w & 63);
            }
        for (int t : ap.wr[i]) writers[t].push_back(i);
        for (int t : ap.rd[i]) if (touch[t].empty() || touch[t].back() != i) touch[t].push_back(i);
        for (int t : ap.wr[i]) if (touch[t].empty() || touch[t].back() != i) touch[t].push_back(i);
    }
    // a group launch sits at its first member's place: no op outside the group may lie between two members in the DAG
    for (auto& g : ap.groups)
        for (int x = 0; x < m; ++x) {
            if (std::find(g.begin(), g.end(), x) != g.end()) continue;
            bool below = false, above = false;
            for (int a : g) { below |= (bool)is_anc(a, x); above |= (bool)is_anc(x, a); }
            if (below && above) return GRNET_ESTATE;
        }
    // earlier(a, b): every op that touches a is a strict ancestor of every op that writes b
    auto earlier = [&](int a, int b) {
        if (touch[a].empty() || writers[b].empty()) return false;
        for (int x : touch[a]) for (int w : writers[b]) if (x == w || !is_anc(x, w)) return false;
        return true;
    };
    std::vector<std::vector<char>> conf(nt, std::vector<char>(nt, 0));
    for (int a = 0; a < nt; ++a)
        for (int b = a + 1; b < nt; ++b)
            if (!earlier(a, b) && !earlier(b, a)) conf[a][b] = conf[b][a] = 1;
    for (auto& g : ap.groups) {
        std::vector<int> w, t;
        for (int i : g) { w.insert(w.end(), ap.wr[i].begin(), ap.wr[i].end()); t.insert(t.end(), ap.wr[i].begin(), ap.wr[i].end()); t.insert(t.end(), ap.rd[i].begin(), ap.rd[i].end()); }
        for (int a : w) for (int b : t) if (a != b) conf[a][b] = conf[b][a] = 1;
    }
    // lower bound: the tensors alive across one node -- written by the node or an ancestor, touched by the node or a descendant -- conflict
    // pairwise, so no layout is smaller than their sum; the largest such sum over the ops and over the groups (each contracted alone).
    auto live_sum = [&](const std::vector<int>& node) {
        int64_t sum = 0;
        for (int t = 0; t < nt; ++t) {
            bool before = false, after = false;
            for (int w : writers[t]) for (int x : node) before |= w == x || is_anc(w, x);
            for (int u : touch[t]) for (int x : node) after |= u == x || is_anc(x, u);
            if (before && after) sum += ap.floats[t];
        }
        return sum;
    };
    int64_t best = 0;
    for (int i = 0; i < m; ++i) best = std::max(best, live_sum({i}));
    for (auto& g : ap.groups) best = std::max(best, live_sum(g));
    ap.bound = kArenaHead + best + kArenaTail;
    ap.full_total = kArenaHead + kArenaTail;
    for (int t = 0; t < nt; ++t) ap.full_total += ap.floats[t];
    ap.off.resize(nt);
    if (!compact_layout) {
        int64_t at = kArenaHead;
        for (int t = 0; t < nt; ++t) { ap.off[t] = at; at += ap.floats[t]; }
        ap.total = ap.full_total;
    } else {
        std::vector<std::vector<int>> adj(nt);
        for (int a = 0; a < nt; ++a) for (int b = 0; b < nt; ++b) if (conf[a][b]) adj[a].push_back(b);
        int64_t tot = 0;
        arena_first_fit(ap.floats, adj, kArenaAlign, ap.off, &tot);
        for (int t = 0; t < nt; ++t) ap.off[t] += kArenaHead;
        ap.total = kArenaHead + tot + kArenaTail;
    }
    ap.final_tenant.assign(nt, 1);
    std::vector<char> shares(nt, 0);
    for (int a = 0; a < nt; ++a)
        for (int b = 0; b < nt; ++b) {
            if (a == b || ap.floats[a] == 0 || ap.floats[b] == 0) continue;
            if (ap.off[a] >= ap.off[b] + ap.floats[b] || ap.off[b] >= ap.off[a] + ap.floats[a]) continue;
            if (conf[a][b]) return GRNET_ESTATE;                 // the assignment broke its own contract
            shares[a] = 1;
            if (!earlier(b, a)) ap.final_tenant[a] = 0;
        }
    for (int t = 0; t < nt; ++t) ap.n_shared += shares[t];
    return 0;
}
void grnet::arena_info(const ArenaPlan& ap, int64_t* info) const {
    info[0] = ap.total * 4; info[1] = ap.full_total * 4; info[2] = ap.bound * 4; info[3] = (int64_t)ap.floats.size(); info[4] = ap.n_shared;
}
std::string grnet::arena_text(const ArenaPlan& ap) const {
    static const char* kinds[] = {"CONV", "SUM", "BILINEAR", "POOL", "TAIL", "SMPL", "CONVERT", "FUSEUP"};
    std::string out;
    for (size_t t = 0; t < ap.floats.size(); ++t) {
        std::string nm = "-";
        for (auto& nv : named) if (nv.second.slot == (int)t) { nm = nv.first; break; }
        out += "tensor " + std::to_string(t) + " " + nm + " " + std::to_string(buffer_floats[t]) + " " + std::to_string(ap.off[t]) + "\n";
    }
    for (size_t i = 0; i < ap.rd.size(); ++i) {
        out += "op " + std::to_string(i) + " " + (i < ops.size() ? kinds[ops[i].kind] : "COPYOUT") + " reads";
        for (int t : ap.rd[i]) out += " " + std::to_string(t);
        out += " writes";
        for (int t : ap.wr[i]) out += " " + std::to_string(t);
        out += "\n";
    }
    for (auto& g : ap.groups) {
        out += "group";
        for (int i : g) out += " " + std::to_string(i);
        out += "\n";
    }
    return out;
}

// ------------------------------------------------------------------ the lane schedule
// Read-after-write producers: per op of `list`, in list order, the earlier ops that wrote (part of) a slot it reads -- in first-seen order,
// each once.  The order is part of the schedule: schedule_lanes() breaks ties by it, analyze_dependencies() emits Op::waits in it.
static std::vector<std::vector<int>> raw_producers(const std::vector<Op>& list) {
    std::vector<std::vector<int>> prod(list.size());
    std::map<int, std::vector<int>> writers;               // slot -> ops that wrote (part of) it
    for (int i = 0; i < (int)list.size(); ++i) {
        for (int b : list[i].rd) {
            auto it = writers.find(b);
            if (it == writers.end()) continue;              // the caller's frames
            for (int w : it->second)
                if (std::find(prod[i].begin(), prod[i].end(), w) == prod[i].end()) prod[i].push_back(w);
        }
        for (int o : list[i].wr) writers[o].push_back(i);
    }
    return prod;
}

// Static list scheduling of the op list onto the kLanes streams.  The plan writes "branch b on lane b",
// which leaves the fuse layer of an HR module as a chain of small launches on the lane of the slowest branch
// (measured: ~210 us per stage-4 module in which mostly one small kernel runs at a time).  Here every op gets an
// estimated duration, and ops are placed earliest-start-first (ties: longest remaining path first) on the lane
// that lets them start first, preferring the lane of their latest producer (no cross-lane event).  Streams are FIFO,
// so the resulting list is both the enqueue order and a topological order; analyze_dependencies() then derives
// the cross-lane events from it exactly as for the hand-written lanes.
void grnet::schedule_lanes(std::vector<Op>& list, int n) const {
    const int m = (int)list.size();
    std::vector<double> est(m), blevel(m, 0.0);
    std::vector<std::vector<int>> deps = raw_producers(list), users(m);
    int prev_tail = -1;
    static const double fix_us = GRNET_AB_F(SCHED_FIX, 6.0);
    static const double hop_us = GRNET_AB_F(SCHED_HOP, 4.0);
    for (int i = 0; i < m; ++i) {
        const Op& op = list[i];
        switch (op.kind) {
            case Op::CONV: {
                const double gf = 2.0 * convs[op.conv_idx].macs_per_frame * n / 1e9;
                est[i] = fix_us + gf / (gf > 20 ? 0.105 : gf > 3 ? 0.085 : 0.060);     // us; GFLOP per us = TFLOP/s / 1000
                // launches that run beside three others (everything between transition1 and the heads): measured in company at 16
                // frames (grnet_op_timeline) the four branch convolutions of a module take 19 / 23 / 22 / 32 us for the SAME FLOPs
                // (56x56 ... 7x7: the 7x7 chain is the long pole of stage 4), the stride-2 and small launches 17-23 us
                if (!convs[op.conv_idx].solo && gf < 3) {
                    const ConvLayer& L = convs[op.conv_idx];
                    est[i] = std::max(est[i], 17.0);
                    if (L.ks == 3 && L.stride == 1 && L.in.c == L.cout) est[i] *= L.in.w == 7 ? 1.45 : L.in.w == 56 ? 0.9 : 1.05;
                }
                break;
            }
            case Op::FUSEUP: est[i] = 18; break;
            case Op::POOL: est[i] = 50; break;
            case Op::TAIL: est[i] = 50; break;
            case Op::SMPL: est[i] = 60; break;
            default: est[i] = 8; break;
        }
        if (op.kind == Op::POOL || op.kind == Op::TAIL || op.kind == Op::SMPL) {   // the tail is a chain on the caller's stream
            if (prev_tail >= 0) deps[i].push_back(prev_tail);
            prev_tail = i;
        }
    }
    for (int i = 0; i < m; ++i)
        for (int d : deps[i]) users[d].push_back(i);
    for (int i = m - 1; i >= 0; --i) {
        double b = 0;
        for (int u : users[i]) b = std::max(b, blevel[u]);
        blevel[i] = b + est[i];
    }
    std::vector<int> pending(m), lane_of(m, 0), order;
    std::vector<double> finish(m, 0.0);
    std::vector<char> done(m, 0);
    for (int i = 0; i < m; ++i) pending[i] = (int)deps[i].size();
    double lane_free[kLanes] = {};
    static const int n_lanes = std::min(kLanes, std::max(1, GRNET_AB(LANES, 4)));
    order.reserve(m);
    for (int step = 0; step < m; ++step) {
        int best = -1, best_lane = 0;
        double best_start = 0;
        for (int i = 0; i < m; ++i) {
            if (done[i] || pending[i]) continue;
            double ready = 0;
            int from = -1;
            for (int d : deps[i])
                if (finish[d] >= ready) { ready = finish[d]; from = d; }
            const bool pinned = list[i].kind == Op::POOL || list[i].kind == Op::TAIL || list[i].kind == Op::SMPL;
            int lane = 0;
            double start = std::max(ready, lane_free[0]);
            if (!pinned && list[i].follow >= 0) {             // shares the stream of the op it follows
                lane = lane_of[list[i].follow];
                start = std::max(ready, lane_free[lane]);
            } else if (!pinned) {
                const int pref = from >= 0 ? lane_of[from] : 0;
                lane = pref;
                start = std::max(ready, lane_free[pref]);
                for (int l = 0; l < n_lanes; ++l) {
                    const double st = std::max(ready, lane_free[l]);
                    if (st + hop_us < start) { start = st; lane = l; }   // a cross-lane hop costs an event
                }
            }
            if (best < 0 || start < best_start - 1e-9 || (start < best_start + 1e-9 && blevel[i] > blevel[best])) {
                best = i; best_lane = lane; best_start = start;
            }
        }
        done[best] = 1;
        lane_of[best] = best_lane;
        finish[best] = best_start + est[best];
        lane_free[best_lane] = finish[best];
        for (int u : users[best]) --pending[u];
        order.push_back(best);
    }
    std::vector<Op> out;
    out.reserve(m);
    for (int i : order) {
        Op op = list[i];
        op.lane = lane_of[i];
        op.waits.clear();
        op.record = false;
        out.push_back(std::move(op));
    }
    if (getenv("GRNET_TRACE")) fprintf(stderr, "[grnet] lane schedule: %d ops, estimated makespan %.0f us (sum of estimates %.0f us)\n", m,
                                       *std::max_element(lane_free, lane_free + kLanes), [&] { double t = 0; for (double e : est) t += e; return t; }());
    list.swap(out);
}

// Cross-lane read-after-write edges -> Op::waits / Op::record and the lanes the caller's stream joins (lane_deps.h).  Of the edges only
// those stay that the lane is not ordered behind already: the happens-before order of the launches, and with it every output bit, is that
// of the full edge set.  The graph recorder reads the same Op::waits, so a captured forward has the reduced edges too.
void grnet::analyze_dependencies(std::vector<Op>& ops, std::vector<hipEvent_t>& op_events) {
    const std::vector<std::vector<int>> producers = raw_producers(ops);
    std::vector<int> lane_of(ops.size());
    for (size_t i = 0; i < ops.size(); ++i) lane_of[i] = ops[i].lane;
    static const int reduce_waits = GRNET_AB(WAIT_REDUCE, 1);   // 0: every cross-lane edge waits and every side lane is joined (the schedule until round 6)
    const lane_deps::Handoffs all = lane_deps::all_cross_lane_waits(lane_of, producers);
    const lane_deps::Handoffs kept = reduce_waits ? lane_deps::reduce_cross_lane_waits(lane_of, producers) : all;
    for (size_t i = 0; i < ops.size(); ++i) {
        ops[i].waits = kept.waits[i];
        ops[i].record = kept.record[i] != 0;
    }
    std::fill(join_lane, join_lane + kLanes, false);
    int joins_all = 0, joins_kept = 0;
    for (size_t l = 1; l < kept.join.size() && l < (size_t)kLanes; ++l) {
        join_lane[l] = kept.join[l] != 0;
        joins_all += all.join[l];
        joins_kept += kept.join[l];
    }
    handoff_counts[GRNET_PLAN_OPS] = (int64_t)ops.size();
    handoff_counts[GRNET_PLAN_WAITS_ALL] = (int64_t)all.n_waits;
    handoff_counts[GRNET_PLAN_RECORDS_ALL] = (int64_t)all.n_records;
    handoff_counts[GRNET_PLAN_WAITS] = (int64_t)kept.n_waits;
    handoff_counts[GRNET_PLAN_RECORDS] = (int64_t)kept.n_records;
    handoff_counts[GRNET_PLAN_LANES_ALL] = joins_all;
    handoff_counts[GRNET_PLAN_LANES_JOINED] = joins_kept;
    op_events.assign(ops.size(), nullptr);
    if (getenv("GRNET_TRACE"))
        fprintf(stderr, "[grnet] dependencies: %zu ops, cross-lane waits %zu -> %zu, recorded events %zu -> %zu, joined lanes %d -> %d\n", ops.size(), all.n_waits,
                kept.n_waits, all.n_records, kept.n_records, joins_all, joins_kept);
}
