// Internal to the runtime (grnet*.cpp), never included from include/: the plan types and `struct grnet`, the handle behind grnet_t.
//   grnet_plan.cpp     the network plan, the arena planner and the lane scheduler -- host code only, no HIP call
//   grnet_weights.cpp  the weight loader (reference state_dict keys -> BN-folded, kernel-layout weights) and its entry points
//   grnet_run.cpp      allocation, kernel choice, the launch path, the graph cache, the tuner
//   grnet_hooks.cpp    the single-op test and timing hooks
//   grnet_render.cpp   the mesh overlay: the face table, grnet_render_meshes and its stage hooks; the render workspace
//   grnet_skeleton.cpp the 3D skeleton view: grnet_render_segments and its two stage hooks, grnet_spin_joints
//   grnet_seq.cpp      shared by the calls over sequences lying back to back: the scratch grower, the entry of the calls that upload a table (seq_call)
//   grnet_bbox.cpp     boxes from 2D joints: grnet_bbox_from_joints2d and its 1-medoid hook
//   grnet_metrics.cpp  pose metrics: grnet_pose_metrics and the Procrustes hook
//   grnet_translation.cpp  the camera-space trajectory: grnet_fit_translation
//   grnet_track.cpp    per-frame boxes from 2D joints: grnet_track_boxes and its two stage hooks
//   grnet_gait.cpp     gait events and parameters from the 3D joints: grnet_gait_parameters and its events hook
//   grnet_kinematics.cpp  joint-angle kinematics per gait cycle: grnet_gait_kinematics and its cycles hook
//   grnet_turns.cpp    turns and straight-walking gait parameters: grnet_gait_turns and its runs hook
//   grnet_contacts.cpp foot contact phases and double support: grnet_gait_contacts and its runs hook
//   grnet_regularity.cpp gait regularity from the autocorrelation: grnet_gait_regularity and its autocorrelation hook
//   grnet_harmonics.cpp harmonic ratios per stride: grnet_gait_harmonics and its stride hook
//   grnet_entropy.cpp  sample entropy at several scales: grnet_gait_entropy and its counting hook
//   grnet_stability.cpp local dynamic stability: grnet_gait_stability and its divergence hook
//   grnet_spectrum.cpp the Welch spectrum: grnet_gait_spectrum and its density hook
//   grnet_recurrence.cpp recurrence quantification: grnet_gait_recurrence and its counting hook
//   grnet_coordination.cpp arm swing and inter-limb coordination: grnet_gait_coordination and its cross-spectrum hook
//   grnet_balance.cpp  footprints, centre of mass and margin of stability: grnet_gait_balance and its steps hook
//   grnet_bootstrap.cpp the gait call's step and stride tables and bootstrap intervals of a per-step table: grnet_gait_step_tables, grnet_bootstrap_table
//   grnet_smoothness.cpp movement smoothness: grnet_gait_smoothness, its slot count and its arc-length hook
//   grnet_body.cpp     mesh volume, centre of mass and second moments: grnet_mesh_moments, its form hook, grnet_faces_closed
//   grnet.cpp          the rest of the C ABI of include/grnet_hip.h
#pragma once
#include "../../include/grnet_hip.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <map>
#include <memory>
#include <optional>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "kernels.h"
#include "seq_args.h"
#include "gait_entropy.h"

namespace grnet_detail {
using namespace grk;

inline uint16_t f32_to_bf16(float f) {                     // round to nearest even, as the kernels do
    uint32_t u;
    memcpy(&u, &f, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
constexpr int kBranchCh[4] = {32, 64, 128, 256};

struct HostTensor {
    std::vector<int64_t> shape;
    std::vector<float> data;
    size_t numel() const { return data.size(); }
};

struct AddRef { View v; int shift; };

struct ConvSeg { std::string wkey, bnprefix, biaskey; int cout; };

struct ConvLayer {
    View in, out;
    std::vector<ConvSeg> segs;
    int cout = 0, ks = 1, stride = 1, relu = 0;
    int relu_from = 0;          // relu applies to output channels >= relu_from (a merged launch whose first segment is linear)
    bool solo = false;          // runs with no other launch beside it (stem, layer1, PARE head): isolated timings predict it well
    int cin_w = 0;              // input channels of the weight tensor (< in.c only for the bf16 stem: 3 of the 8 stored)
    std::vector<AddRef> adds;
    float* w_dev = nullptr;
    float* b_dev = nullptr;
    float* wino4_dev = nullptr; // transformed weights [36][cin_pad][cout_pad] of the Winograd F(4x4,3x3) kernel (the widest 56x56 layers only)
    float* stem_dev = nullptr;   // flattened-K weights of the stem's first convolution (conv_stem.hip)
    float* wino4s_dev = nullptr; // transformed weights of the register-resident F(4x4,3x3) kernel of the 14x14 / 7x7 maps (conv_wino4s.hip)
    int cin_pad = 0, cout_pad = 0;
    double macs_per_frame = 0;
    int lane_hint = 0;          // lane of this convolution when it is launched on its own (not as a group member)
    View in2;                   // bf16: second input of a merged 1x1 launch (layer1.0: conv3 over t and the downsample over x as ONE GEMM); in2.c == 0: none
    ConvSeg seg2;               // its weights / BatchNorm (same output channels, summed)
    int pair_next = -1, pair_of = -1;   // bf16 layer1: this 64 -> 256 expansion also runs convolution pair_next (the next Bottleneck's 256 -> 64 reduction) from its tile / this
                                        // reduction runs inside the launch of convolution pair_of (large calls: pair_active())
    int chain = -1, chain_pos = 0;   // bf16: member chain_pos of BasicBlock chain `chain` (conv_bf16_chain.hip); position 0 launches the whole chain in large calls
    int roll = -1, roll_pos = 0;     // bf16: member roll_pos of the row-walking launch `roll` (conv_bf16_roll.hip: the stem pair, a layer1 Bottleneck); position 0 launches it in large calls
    std::map<int, int> tuned;   // n_frames -> launch configuration (tile hint) measured fastest by grnet_tune
};

// The up half of one HR module's fuse layer (hr_fuse.hip): outputs 0 .. nb-2 in one launch.
struct FuseUpPlan {
    int nb = 0;
    std::string prefix;                  // "backbone.stage3.1."
    std::vector<View> xs;                // the module's branch outputs (nb)
    std::vector<View> outs;              // outputs 0 .. nb-2 (final)
    std::vector<std::vector<View>> extra; // per output: the finished down chains D_ij, j < i, added by the grouped launch
    float* w_dev[3][3] = {};             // [output i][source j - i - 1], pack_fuse_up_weights
    float* b_dev[3] = {};                // [output i]: sum over j of the folded BatchNorm shifts
    double macs_per_frame = 0;
    int only = -1;                       // >= 0: this plan finishes output `only` alone (bf16: one launch per output, each on its branch's lane)
};

// The 8 convolutions (4 BasicBlocks) of one branch of one HR module, runnable as ONE launch on the bf16 path (conv_bf16_chain.hip).
struct ChainPlan {
    std::vector<int> convs;              // indices into grnet::convs, in execution order
    int c = 0, w = 0;
};

// Layers that run as ONE row-walking launch on the bf16 path in large calls (conv_bf16_roll.hip)
struct RollPlan {
    int kind = 0;                        // 0: stem pair (conv1, conv2); 1: layer1.0 (conv1, conv2, conv3 over [u ; x]); 2: layer1.1-3 (conv1, conv2, conv3 + residual)
    std::vector<int> convs;              // indices into grnet::convs, in execution order
};

struct Op {
    enum Kind { CONV, SUM, BILINEAR, POOL, TAIL, SMPL, CONVERT, FUSEUP } kind;
    int conv_idx = -1;
    SumArgs sum{};
    View bin, bout;   // bilinear
    // multi-lane execution: independent branches of the HR modules run on parallel HIP streams
    // (captured as parallel branches of the hipGraph); cross-lane read-after-write edges are events
    int lane = 0;
    int follow = -1;          // plan index of an op this one depends on and whose stream it must share (the lane scheduler keeps them together)
    std::vector<int> waits;   // ops (on other lanes) whose completion event this op waits for
    bool record = false;      // some op on another lane consumes this op's output
    std::vector<int> rd, wr;  // planned buffers (slot indices) the op reads / writes (annotate_plan): dependency tracking is keyed on these, never on addresses
};

// What plan_arena() works out for one layout of the activation arena (the sharing rule is stated there, grnet_plan.cpp).
struct ArenaPlan {
    std::vector<int64_t> floats;        // per slot, at max_frames, 256-byte aligned
    std::vector<int64_t> off;           // floats from the arena's base (the leading zero block included)
    int64_t total = 0, full_total = 0, bound = 0;   // floats, head and tail blocks included
    int n_shared = 0;
    std::vector<char> final_tenant;     // nothing is placed over the slot's bytes later in the forward
    std::vector<std::vector<int>> groups;   // op indices (plan order) some launch form runs as one launch
    std::vector<std::vector<int>> rd, wr;   // per op, + the virtual copy-out op at the end
};

constexpr int kLanes = 8;            // streams available to the lane scheduler (the hand-written plan uses 4)

// Every entry point runs on the handle's device whatever the caller's current device is, and leaves the caller's device as it found it.
// The few-row GEMMs borrow split-K scratch through a thread-local pointer (set_gemm_workspace); this lease takes it back on every
// exit path, so a failed call never leaves the pointer aimed at scratch the handle may free later.
struct GemmWorkspaceLease {
    GemmWorkspaceLease(float* ws, size_t floats) { set_gemm_workspace(ws, floats); }
    ~GemmWorkspaceLease() { set_gemm_workspace(nullptr, 0); }
    GemmWorkspaceLease(const GemmWorkspaceLease&) = delete;
    GemmWorkspaceLease& operator=(const GemmWorkspaceLease&) = delete;
};
// The same for the tap sink of an armed temporal call: installed for the launchers of that call, gone on every way out of it.
struct TapLease {
    explicit TapLease(TapSink* t) { g_taps = t; }
    ~TapLease() { g_taps = nullptr; }
    TapLease(const TapLease&) = delete;
    TapLease& operator=(const TapLease&) = delete;
};

struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};

// Offsets for n buffers of which some pairs may not overlap (grnet_arena_assign, plan_arena): grnet_plan.cpp
void arena_first_fit(const std::vector<int64_t>& sizes, const std::vector<std::vector<int>>& adj, int64_t align, std::vector<int64_t>& off, int64_t* total);

// The render workspace, shared by the mesh overlay and the skeleton view (grnet_render.cpp): [depth words | vertex records of kRasterSlots meshes]
constexpr int kSmplVerts = 6890;
constexpr size_t kRasterDepthWords = (size_t)kRasterMaxDim * kRasterMaxDim;   // the depth images of a launch group share ONE largest image: 128 MiB
size_t raster_record_bytes(int slots, int V);
bool raster_dims_ok(int H, int W);
struct DeviceBlock {                                        // freed when a hook returns, whichever way
    void* p = nullptr;
    ~DeviceBlock() { if (p) (void)hipFree(p); }
};

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) return fail(GRNET_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

}  // namespace grnet_detail

using namespace grk;
using namespace grnet_detail;
using namespace seq_args;

struct grnet {
    // ------------------------------------------------------------------ the handle: what it was created for, its state, its options
    int device = 0, max_frames = 0;
    int dtype = 0;               // 0: fp32 NCHW activations, 1: bf16 NHWC activations (conv_bf16.hip), fp32 tail either way
    bool compact = false;        // GRNET_CREATE_COMPACT_ARENA
    bool finalized = false, smpl_loaded = false, gru_ready = false, tsattn_ready = false, featcorr_ready = false;
    std::string err;
    bool use_graph = false;
    bool multi_lane = true;
    int conv_tile_hint = 0;
    int wino_mode = 1;                               // GRNET_OPT_WINOGRAD: 1 = the eligible 3x3 layers on 56x56 maps run the Winograd kernel
    static constexpr int kChainModeAll = 1023;
    int chain_mode = (getenv("GRNET_BF16_CHAIN") ? atoi(getenv("GRNET_BF16_CHAIN")) : kChainModeAll) & kChainModeAll;     // GRNET_OPT_BF16_CHAIN: bits 0-3 BasicBlock chains by branch, 4 wide bands, 5 stride-2 bands, 6 layer1 1x1 pairs, 7 1x1 stream kernel
    int bf16_min_frames = 0;                         // GRNET_OPT_BF16_MIN_FRAMES: 0 = every kernel group of chain_mode from its own smallest call (64 / 32 / 64 / 19 / 42 frames), else from this many
    // GRNET_OPT_GRU_MODE (gru_kernels.hip): 3 = rows-per-wave split recurrence with v_exp / v_rcp gates (default), 2 = the same with expf / tanhf,
    // 1 = round 3's column slices, 0 = one workgroup per (sequence, direction); + 16: agent-scope granule stores whatever the placement.
    // gru_fault: one host-mapped word the split kernels set when a hand-off poll hits its bound (an XCD-placement or memory-scope assumption broke:
    // round-5 advice).  The next temporal call sees it WITHOUT a synchronisation, reports GRNET_ESTATE once and moves the handle to agent-scope stores.
    int gru_mode = 3;
    unsigned* gru_fault = nullptr;        // host pointer (hipHostMalloc, mapped)
    unsigned* gru_fault_dev = nullptr;    // the same word as the device sees it

    // ------------------------------------------------------------------ the plan (build_plan, grnet_plan.cpp)
    std::vector<ConvLayer> convs;
    std::vector<Op> ops;        // the plan in the order it is written (build_plan)
    std::vector<size_t> buffer_floats;   // planned buffers in creation order (View::slot indexes it): floats per image
    std::vector<FuseUpPlan> fuse_ups;
    std::vector<ChainPlan> chains;
    std::vector<RollPlan> rolls;
    struct SumPlan { View out; std::vector<AddRef> adds; };   // Op::SUM: out = relu(sum of the addends)
    std::vector<SumPlan> sum_views;
    std::vector<std::pair<std::string, View>> named;   // intermediate tensors exposed to grnet_debug_tensor
    std::vector<int> end_reads;      // read after the op list by the forward's copy-outs (conv_out / copy_out): cat, heat, smpl_feats
    // named views for outputs / debug
    View v_input, v_cat, v_heat, v_smpl_feats, v_csmap;
    View v_in8;                  // bf16 without conv_bf16_stem: the caller's frames converted to NHWC bf16 with 8 channels (3 real)
    bool bf16_stem = false;
    int cur_lane = 0;
    bool solo_region = false;   // build_plan: convolutions added now are part of a chain nothing else overlaps

    // ------------------------------------------------------------------ the activation arena (plan_arena, grnet_plan.cpp) and the device memory of the handle
    static constexpr int64_t kArenaHead = 64, kArenaTail = 64, kArenaAlign = 64;   // floats: the zero block, conv_wino4s_f32's masked over-read, 256-byte buffers
    ArenaPlan arena_plan;
    float* arena = nullptr;
    size_t arena_floats = 0;
    std::vector<void*> dev_allocs;
    float* zeros = nullptr;
    float *d_plf = nullptr, *d_csf = nullptr, *d_stats = nullptr, *d_rot6d = nullptr, *d_shape = nullptr, *d_cam = nullptr;
    float *d_rotmat = nullptr, *d_theta = nullptr, *d_A = nullptr, *d_verts = nullptr, *d_kp3d = nullptr, *d_kp2d = nullptr;

    // ------------------------------------------------------------------ weights (grnet_weights.cpp)
    std::unordered_map<std::string, HostTensor> tensors;
    TailWeights tailw{};
    SmplTables smpl{};
    GruWeights gruw{};
    TsAttnWeights tsw{};
    FeatCorrWeights fcw{};
    std::vector<float> J_regressor_host;
    // grnet_set_joint_regressor: the selected rows in MFMA fragment order and the slice partials of grnet_regress_joints (max_frames frames)
    float *jreg_pack = nullptr, *jreg_ws = nullptr;
    int jreg_rows = 0;
    // grnet_smooth_pose: rotations (max_frames,24,9) | betas (max_frames,10) | kp (max_frames,29,3), allocated at the first call, outside the arena
    float* smooth_ws = nullptr;
    // grnet_load_faces: the face table with its vertex -> face rows (one device block); grnet_render_meshes: the vertex records and depth images of
    // up to kRasterSlots meshes, allocated at the first call, outside the arena (grnet_render.cpp)
    RasterMesh rmesh{};
    void* rmesh_block = nullptr;
    void* raster_ws = nullptr;
    // grnet_mesh_moments / grnet_faces_closed: the table as grnet_load_faces took it, and its directed edges that are duplicated or lack their
    // reverse (DESIGN 4.25 rule 5; < 0: not counted since the table was loaded) -- grnet_body.cpp
    std::vector<int32_t> faces_host;
    long long faces_unmatched = -1;
    // grnet_render_segments: the segment table of a call goes to the device through pinned host memory, a ring of kSegStageSlots tables each with
    // the event recorded behind its copy, so the call enqueues and returns (grnet_skeleton.cpp)
    static constexpr int kSegStageSlots = 4;
    void* seg_stage = nullptr;
    hipEvent_t seg_stage_done[kSegStageSlots] = {};
    unsigned seg_stage_next = 0;

    // grnet_bbox_from_joints2d / grnet_op_medoid: points, heights and the row sums' partials; the calls of seq_call: their table and what lies
    // behind it.  Grown on demand, outside the arena (grow_scratch)
    void* bbox_ws = nullptr;
    size_t bbox_ws_bytes = 0;

    // grnet_pose_metrics: the sequences' sums and counts (and the per-frame rows when the caller takes none), grown on demand, outside the arena.
    // A buffer of its own: a metrics call and a box call on two streams never meet in one
    void* metric_ws = nullptr;
    size_t metric_ws_bytes = 0;

    // ------------------------------------------------------------------ the schedule, the tuning tables and the graph cache (grnet_run.cpp)
    std::vector<Op> ops_flat;   // the same ops placed on the lane streams by schedule_lanes(): the enqueue order
    std::vector<hipEvent_t> op_events_flat;
    hipStream_t side[kLanes] = {};      // lanes 1.. (lane 0 = the caller's stream)
    hipEvent_t ev_fork = nullptr, ev_join[kLanes] = {};
    int lanes_used = 1;
    bool join_lane[kLanes] = {};        // the caller's stream waits for this side lane after the op list: its last op is not already behind lane 0's (analyze_dependencies)
    int64_t handoff_counts[GRNET_PLAN_COUNTS] = {};   // grnet_plan_counts, indexed by the GRNET_PLAN_* enumerators
    int launches_last = 0;
    int last_n = 16;                   // frame count of the latest forward (grnet_conv_executed_flops_per_frame reports for it)
    std::map<int, int> tuned_mode;     // n -> bit 0: measured per-shape configurations (else cost model), bit 2: eager launches on the lane streams even if graphs are enabled
    struct GraphKey {
        int n; const void* in; grnet_outputs_t o;
        bool operator<(const GraphKey& r) const {
            if (n != r.n) return n < r.n;
            if (in != r.in) return in < r.in;
            return std::memcmp(&o, &r.o, sizeof(o)) < 0;
        }
    };
    struct GraphEntry { hipGraphExec_t exec; unsigned long long last_use; };
    std::map<GraphKey, GraphEntry> graphs;                  // at most kMaxGraphs captured forwards, least recently used evicted
    unsigned long long graph_clock = 0;
    std::vector<GraphKey> seen_once;
    hipStream_t capture_stream = nullptr;   // the caller's stream may be the (uncapturable) null stream
    // diagnostic (grnet_op_timeline): timing events around every op of one eager forward
    std::vector<hipEvent_t>* tl_start = nullptr;
    std::vector<hipEvent_t>* tl_end = nullptr;

    // ------------------------------------------------------------------ the temporal modules (grnet.cpp)
    // Scratch of the temporal modules (GRU, attention block, feature corrector): owned by the handle and grown on demand, so a call
    // with a size seen before allocates nothing (graph-capturable, no allocator traffic per call).  Growing synchronises the device.
    float* temporal_ws = nullptr;
    size_t temporal_ws_floats = 0;
    // grnet_temporal_taps: armed for the NEXT temporal call only; that call checks the buffer against what it will copy before it enqueues anything,
    // installs the sink for its launchers (TapLease) and leaves the layout of what it copied in tap_sink.layout for grnet_temporal_tap_layout
    TapSink tap_sink;
    bool taps_armed = false;

    // ================================================================== inline: what the launch path calls per op
    int fail(int code, const std::string& msg) {
        err = msg;
        return code;
    }
    static View slice(View v, int coff, int c) {
        v.coff += coff;
        v.c = c;
        return v;
    }
    void name_view(const std::string& n, const View& v) { named.emplace_back(n, v); }
    // A view becomes an address here, at the launch, and nowhere else: the base (image 0, channel 0) of its buffer in the arena, or `frames` (only
    // ever read) for the caller's frames.  Meaningful on an allocated handle only: the host-only plans of grnet_arena_query / grnet_arena_layout have no arena.
    float* base(const View& v, const float* frames = nullptr) const {
        if (v.slot >= 0) return arena + arena_plan.off[v.slot];
        return v.slot == View::kFrames ? const_cast<float*>(frames) : nullptr;
    }
    // ... and the (pointer, ctot, coff) triple of a kernel argument struct (float or void pointers: a bf16 handle keeps NHWC bf16 behind the same fields)
    template <class P>
    void bind(const View& v, P*& p, int& ctot, int& coff, const float* frames = nullptr) const { p = base(v, frames); ctot = v.ctot; coff = v.coff; }
    const void* bf16_at(const View& v) const { return reinterpret_cast<const uint16_t*>(base(v)) + v.coff; }   // first channel of an NHWC bf16 view
    // bf16 layer1: expansion + next reduction as one launch from 19 frames per call on (the 256-channel tile needs >= 512 workgroups of 112 pixels); bit 6 of the
    // GRNET_OPT_BF16_CHAIN mask.  A forced tile switches it off.
    bool pair_active(int n) const { return dtype == 1 && (chain_mode & 64) && !conv_tile_hint && (long)n * 56 * 56 >= 256L * 112 * 2; }      // (geometric: GRNET_OPT_BF16_MIN_FRAMES does not lower it)

    // ================================================================== grnet_plan.cpp: runs without a device
    View new_buffer(int c, int h, int w);
    View add_conv(View in, std::vector<ConvSeg> segs, int ks, int stride, bool relu, std::vector<AddRef> adds = {}, const View* out_override = nullptr);
    View conv_bn(View in, const std::string& wkey, const std::string& bn, int cout, int ks, int stride, bool relu, std::vector<AddRef> adds = {},
                 const View* out_override = nullptr);
    View add_bilinear(View in);
    std::vector<View> hr_module(std::vector<View> xs, const std::string& p, const View* out0);
    std::vector<View> hr_fuse_grouped(const std::vector<View>& xs, const std::string& p, const View* out0, const std::vector<int>& branch_tail);
    std::vector<View> hr_fuse_separate(std::vector<View> xs, const std::string& p, const View* out0, bool up0 = false, const std::vector<int>& branch_tail = {});
    void add_roll(int kind, int n_convs);
    void build_plan();
    void op_reads(const Op& op, std::vector<int>& r) const;
    void op_writes(const Op& op, std::vector<int>& w) const;
    void annotate_plan();
    std::string op_label(const Op& op) const;
    std::vector<std::vector<int>> launch_groups() const;
    int plan_arena(bool compact_layout, ArenaPlan& ap) const;
    void arena_info(const ArenaPlan& ap, int64_t* info) const;
    std::string arena_text(const ArenaPlan& ap) const;
    void schedule_lanes(std::vector<Op>& list, int n) const;
    void analyze_dependencies(std::vector<Op>& ops, std::vector<hipEvent_t>& op_events);

    // ================================================================== grnet_weights.cpp
    const HostTensor* find(const std::string& k) const;
    int upload(const std::vector<float>& h, float** d);
    int upload_key(const std::string& k, size_t numel, const float** d);
    int pack_conv(ConvLayer& L);
    int pack_fuse_up(FuseUpPlan& fp);
    int finalize_gru();
    int finalize_tsattn();
    int finalize_featcorr();
    int finalize();

    // ================================================================== grnet_run.cpp
    int allocate();
    int install_schedule(int n);
    // Which kernel runs convolution L in a call of n frames: ONE place, used by the launcher, by the executed-FLOP report and by the
    // per-kernel table of bench.py (round-3 review: the report read a hidden "latest n" and ignored the environment masks).
    enum ConvKernel { K_BF16, K_BF16_STEM, K_BF16_ROLL, K_BF16_ROLL_MEMBER, K_BF16_CHAIN, K_BF16_CHAIN_MEMBER, K_BF16_PAIR, K_BF16_PAIR_MEMBER, K_BF16_WIDE, K_BF16_S2, K_WINO4S, K_PW, K_STEM, K_WINO4, K_DIRECT };
    int hint_for(const ConvLayer& L, int n) const;
    bool wino4s_runs(const ConvLayer& L, int n) const;
    bool pw_on(const ConvLayer& L) const;
    int bf16_from(int dflt) const;
    bool chain_active(const ChainPlan& c, int n) const;
    bool wide_runs(const ConvLayer& L, int n) const;
    bool s2_runs(const ConvLayer& L, int n) const;
    bool roll_active(const RollPlan& r, int n) const;
    ConvKernel kernel_for(const ConvLayer& L, int n) const;
    double executed_ratio(const ConvLayer& L, int n) const;
    std::string kernel_name(const ConvLayer& L, int n) const;
    int launch_form(const ConvLayer& L, int n, std::string* out);
    bool tap_written(const View& v) const;
    ConvArgs conv_args(const ConvLayer& L, const float* frames, int n) const;
    int launch_conv_op(const ConvLayer& L, const float* frames, int n, hipStream_t s, int* n_launches);
    int launch_fuse_up_op(const FuseUpPlan& fp, int n, hipStream_t s);
    struct HeadOutputs { float *rot6d, *rotmat, *theta, *verts, *kp3d, *kp2d; };
    HeadOutputs head_outputs(const grnet_outputs_t& o) const;
    int enqueue(const float* frames, int n, const grnet_outputs_t& o, hipStream_t s, bool convs_only = false);
    int forward(const float* frames, int n, const grnet_outputs_t* out, hipStream_t s);
    void drop_graphs();
    int tune(int n, hipStream_t s, int level = 1);
    int head_from_feats(const float* plf, const float* csf, int n, const grnet_outputs_t& o, hipStream_t s);
    int gait_correct(const float* plf, const float* csf, const float* cam, int cam_ld, const float* bbox, const float* cimg, int b, int T,
                     const grnet_outputs_t& o, const grnet_gait_outputs_t& g, hipStream_t s);
    int op_timeline(const float* frames, int n, hipStream_t s, std::string& text);

    // ================================================================== grnet_hooks.cpp
    int op_conv2d_bf16(const float* in_dev, int n, int cin, int hgt, int wid, const float* w_host, const float* bias_host, int cout, int ks,
                       int stride, int relu, const float* add_dev, float* out_dev, int tile_hint, hipStream_t s);
    int op_conv2d_bf16_adds(const float* in_dev, int n, int cin, int hgt, int wid, const float* w_host, const float* bias_host, int cout, int ks, int stride,
                            int relu, int n_add, const float* const* adds_dev, const int* add_ctot, const int* add_coff, const int* add_shift, float* out_dev,
                            int tile_hint, hipStream_t s);
    int op_conv_chain_bf16(const float* in_dev, int n, int c, int wid, int nconv, const float* w_host, const float* bias_host, float* out_dev, int reps,
                           float* us_out, hipStream_t s);

    // ================================================================== grnet.cpp
    ~grnet();
    int dev_alloc(float** p, size_t floats);
    void jreg_clear();
    void faces_clear();
    int seg_stage_slot(void** slot, hipEvent_t* done);   // grnet_skeleton.cpp: the next table of the ring, free to be written
    int grow_scratch(void*& ws, size_t& have, size_t bytes, const char* what, char** out);   // grnet_seq.cpp: ws of at least this size
    int bbox_scratch(size_t bytes, char** out) { return grow_scratch(bbox_ws, bbox_ws_bytes, bytes, "box workspace", out); }
    int metric_scratch(size_t bytes, char** out) { return grow_scratch(metric_ws, metric_ws_bytes, bytes, "metric workspace", out); }
    int raster_workspace(const char* who);   // grnet_render.cpp: raster_ws, allocated at the first call of grnet_render_meshes(_ex) or grnet_render_segments
    const Op* nth_conv_op(int pos) const;
    int gru_fault_check();
    int taps_begin(size_t need, const char* what);
    int temporal_scratch(size_t floats, float** out);
    static size_t gru_ws_floats(size_t rows, int b);
    GruWorkspace gru_carve(float* p, size_t rows, int b, float** xc) const;
    int clip_limit(int n, const char* tail);
};

// grnet_seq.cpp: the calls whose kernels read the sequences' offsets and the Gaussian's weights from the device (per-frame boxes, gait, kinematics
// and their hooks).  The first kSeqFront bytes of such a call's scratch (bbox_ws) hold its table -- the weights (host-made, scipy's), then the
// n_seq + 1 frame offsets -- uploaded through one slot of the pinned ring, so the copy is enqueued like a kernel.
constexpr size_t kSeqOffsetsAt = align256((size_t)(kTrackMaxRadius + 1) * sizeof(double));      // the weights lie in front: the copy ends with the offsets
constexpr size_t kSeqFront = align256(kSeqOffsetsAt + (size_t)(kTrackMaxSeqs + 1) * sizeof(int32_t));
struct SeqCall {
    std::optional<DeviceGuard> guard;      // held until the call's launches are enqueued
    const int* off = nullptr;              // on the device
    const double* weights = nullptr;       // on the device
    int radius = -1;                       // < 0: sigma == 0, no Gaussian
    char* behind = nullptr;                // the call's `extra` bytes of scratch, behind the table
};
int seq_call_check(grnet* h, const std::string& name, const int32_t* off, int n_seq, long long unit);      // the two halves of seq_call
int seq_call_upload(grnet* h, const std::string& name, const int32_t* off, int n_seq, double sigma, size_t extra, hipStream_t s, SeqCall* c);
inline size_t seq_no_extra(int) { return 0; }      // the `extra` of a call that keeps nothing behind its table
// The entry of such a call, after its own argument checks: n_seq within [1, kTrackMaxSeqs] and the offsets' rules (seq_args.h, `unit` values per
// frame), then the device guard, kSeqFront + extra(frames) bytes of scratch and the table, staged and enqueued on `s`.  `extra` is asked for
// the sizes only once the offsets hold, so it may trust its frame count.
template <class Extra>
int seq_call(grnet* h, const std::string& name, const int32_t* off, int n_seq, long long unit, double sigma, hipStream_t s, SeqCall* c, Extra extra) {
    if (int rc = seq_call_check(h, name, off, n_seq, unit)) return rc;
    return seq_call_upload(h, name, off, n_seq, sigma, extra(off[n_seq]), s, c);
}
// The same for a call whose work is quadratic in a sequence's frames (sample entropy, local dynamic stability, and their hooks): the refusal of a
// sequence of more than kEntMaxFrames frames (gait_entropy.h's ent_long_sequence) stands between the two halves, in ONE sentence for all of them.
template <class Extra>
int ent_seq_call(grnet* h, const std::string& name, const int32_t* off, int n_seq, long long unit, double sigma, hipStream_t s, SeqCall* c, Extra extra) {
    if (int rc = seq_call_check(h, name, off, n_seq, unit)) return rc;
    const int q = grk::ent_long_sequence(off, n_seq);
    if (q >= 0)
        return h->fail(GRNET_EINVAL, name + "sequence " + std::to_string(q) + " has " + std::to_string(off[q + 1] - off[q]) + " frames, more than " +
                                         std::to_string(grk::kEntMaxFrames) + " (the work is quadratic in them)");
    return seq_call_upload(h, name, off, n_seq, sigma, extra(off[n_seq]), s, c);
}
