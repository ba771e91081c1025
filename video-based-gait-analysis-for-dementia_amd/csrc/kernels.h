// Internal launch interface between the runtime (grnet_impl.h: the plan of grnet_plan.cpp, the launch path of grnet_run.cpp) and the HIP kernels.
// Activations live in HBM as fp32 NCHW (fp32 handles) or bf16 NHWC with channels padded to a multiple of 8
// (bf16 handles; the tail after the pooling is fp32 either way).  A View names a channel slice [coff, coff+c)
// of a planned buffer that holds ctot channels per image, so producers write straight into their slice of
// the 480-channel concat buffer (reference: torch.cat, hrnet.py:524) with no copy kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "raster_lines.h"
#include "seq_args.h"

#include <initializer_list>
#include <mutex>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

// ---- environment switches ------------------------------------------------------------------------------------------------------------
// The product library reads FIVE environment variables, all documented in include/grnet_hip.h ("Environment"): GRNET_TRACE, GRNET_RCCL_LIB,
// GRNET_MULTI_LANE, GRNET_WINO, GRNET_BF16_CHAIN (the last three are the process-wide defaults of grnet_set_option values).  Every other
// A/B switch of the kernels and of the plan is a GRNET_AB(NAME, default): the default as a compile-time constant in the product build -- a
// stray GRNET_* variable cannot change kernels, numerics or the schedule there (tests/test_host_cpu.py greps for getenv, tests/
// test_gpu_options.py sets retired variables and compares bits) -- and read from the environment variable GRNET_<NAME> only in diagnostic
// builds (`make ABLATION=1 BUILD=build_abl LIB=../libgrnet_hip_abl.so`, loaded by tools/ through GRNET_LIB_PATH).
#ifdef GRNET_ABLATION
#include <cstdlib>
#define GRNET_AB(name, dflt) (getenv("GRNET_" #name) ? atoi(getenv("GRNET_" #name)) : (dflt))
#define GRNET_AB_F(name, dflt) (getenv("GRNET_" #name) ? atof(getenv("GRNET_" #name)) : (dflt))
#define GRNET_AB_SET(name) (getenv("GRNET_" #name) != nullptr)
#define GRNET_AB_STR(name) getenv("GRNET_" #name)
#else
#define GRNET_AB(name, dflt) (dflt)
#define GRNET_AB_F(name, dflt) (dflt)
#define GRNET_AB_SET(name) false
#define GRNET_AB_STR(name) (static_cast<const char*>(nullptr))
#endif

// launchers: pass a failed HIP call's error on to the caller
#define GRK_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return _e; } while (0)

namespace grk {

// One-time work per device (kernel attributes, device queries) that launchers used to cache in plain function-local statics: two host
// threads driving two handles raced on those (a thread could see the flag set before the other's hipFuncSetAttribute had finished).
// Only SUCCESS is cached (round-4 advice: one transient failure used to disable a kernel family for the life of the process): a failed
// attempt is retried by the next launch.  Device ids index a small vector grown under the lock.
struct PerDeviceOnce {
    std::mutex m;
    std::vector<char> done;
    std::vector<int> val;
};
inline hipError_t current_device(int* dev) {
    return (hipGetDevice(dev) != hipSuccess || *dev < 0) ? hipErrorInvalidDevice : hipSuccess;
}
template <typename F>
hipError_t once_per_device(PerDeviceOnce& c, int dev, F&& f, int* value = nullptr) {      // f(int* value) -> hipError_t
    std::lock_guard<std::mutex> lock(c.m);
    if ((size_t)dev >= c.done.size()) { c.done.resize(dev + 1, 0); c.val.resize(dev + 1, 0); }
    if (!c.done[dev]) {
        int v = 0;
        const hipError_t e = f(&v);
        if (e != hipSuccess) return e;
        c.val[dev] = v;
        c.done[dev] = 1;
    }
    if (value) *value = c.val[dev];
    return hipSuccess;
}
inline hipError_t device_cu_count(int* cus) {                        // CUs of the current device
    static PerDeviceOnce c;
    int dev = 0;
    hipError_t e = current_device(&dev);
    if (e != hipSuccess) return e;
    return once_per_device(c, dev, [&](int* v) { return hipDeviceGetAttribute(v, hipDeviceAttributeMultiprocessorCount, dev); }, cus);
}

// Every kernel launch of the library goes through launch_k().  Normally it is a plain launch on the
// given stream; while a GraphRecorder is installed (grnet_run.cpp builds the per-forward hipGraph with the
// explicit node API, one parallel branch per lane) it appends a kernel node that depends on
// `rec->deps` instead, and leaves {that node} as the dependency of the next launch of the same op.
struct GraphRecorder {
    hipGraph_t graph = nullptr;
    std::vector<hipGraphNode_t> deps;
    int nodes = 0;
    // edge_order != 0: nodes are created WITHOUT dependencies and the edges added afterwards, all lane-chain edges (a launch -> the next launch of its lane)
    // before the cross-lane ones (1) or after them (2): ROCm's executor walks a node's children in insertion order and keeps the first one on the
    // parent's stream, so the order decides whether a lane of the plan stays one stream of the replay
    int edge_order = 0;
    int n_chain = 0;                                   // how many of the leading entries of `deps` are lane-chain predecessors (0 or 1)
    std::vector<hipGraphNode_t> chain_from, chain_to, cross_from, cross_to;
};
extern thread_local GraphRecorder* g_recorder;

template <typename... KArgs, typename... Args, size_t... I>
hipError_t launch_k_impl(void (*kern)(KArgs...), dim3 grid, dim3 block, size_t shmem, hipStream_t s,
                         std::index_sequence<I...>, Args&&... args) {
    if (!g_recorder) {
        hipLaunchKernelGGL(kern, grid, block, shmem, s, std::forward<Args>(args)...);
        return hipGetLastError();
    }
    std::tuple<KArgs...> vals{static_cast<KArgs>(args)...};     // exact parameter types, copied by AddKernelNode
    void* ptrs[] = {static_cast<void*>(&std::get<I>(vals))...};
    hipKernelNodeParams p{};
    p.func = reinterpret_cast<void*>(kern);
    p.gridDim = grid;
    p.blockDim = block;
    p.sharedMemBytes = (unsigned)shmem;
    p.kernelParams = ptrs;
    p.extra = nullptr;
    hipGraphNode_t node = nullptr;
    GraphRecorder& r = *g_recorder;
    hipError_t e = r.edge_order ? hipGraphAddKernelNode(&node, r.graph, nullptr, 0, &p) : hipGraphAddKernelNode(&node, r.graph, r.deps.data(), r.deps.size(), &p);
    if (e != hipSuccess) return e;
    if (r.edge_order)
        for (size_t i = 0; i < r.deps.size(); ++i) {
            const bool chain = (int)i < r.n_chain;
            (chain ? r.chain_from : r.cross_from).push_back(r.deps[i]);
            (chain ? r.chain_to : r.cross_to).push_back(node);
        }
    r.deps.assign(1, node);                            // a second launch of the same op follows the first on its lane
    r.n_chain = 1;
    ++r.nodes;
    return hipSuccess;
}
template <typename... KArgs, typename... Args>
hipError_t launch_k(void (*kern)(KArgs...), dim3 grid, dim3 block, size_t shmem, hipStream_t s, Args&&... args) {
    static_assert(sizeof...(KArgs) == sizeof...(Args), "kernel argument count mismatch");
    return launch_k_impl(kern, grid, block, shmem, s, std::index_sequence_for<KArgs...>{}, std::forward<Args>(args)...);
}

// Plan-side only (no kernel sees one): a view holds the identity of its buffer, never an address.  The handle turns it into
// the buffer's base (image 0, channel 0) at the launch: grnet::base().
struct View {
    static constexpr int kNone = -1;     // no buffer
    static constexpr int kFrames = -2;   // the caller's frames: the pointer each forward is given
    int slot = kNone;     // planned buffer, numbered in creation order (grnet::new_buffer)
    int ctot = 0;         // channels per image in the underlying buffer
    int coff = 0;         // first channel of this view
    int c = 0, h = 0, w = 0;
};

constexpr int kMaxAdd = 3;
constexpr int kConvCK = 8;      // input channels staged per K-chunk

// One fused convolution: out = act( conv(in, w) + bias + sum_k nearest_up(add_k, 2^shift_k) ).
// BatchNorm (eval) is folded into w / bias on the host in fp64 (reference: conv -> BN,
// hrnet.py:46-52; folding is exact up to fp32 rounding of the folded weights).
struct ConvArgs {
    const float* in; int in_ctot, in_coff;
    int N, Cin, H, W;
    float* out; int out_ctot, out_coff;
    int Cout, Ho, Wo;
    const float* w;            // packed [KS*KS][CinPad][CoutPad], BN scale folded in
    const float* bias;         // [CoutPad], BN shift (+ conv bias) folded in
    int CinPad, CoutPad;
    int ks, stride, relu;
    int relu_from;             // with relu: output channels >= relu_from get the ReLU (0: all) -- merged launches whose first segment is linear (direct kernels only)
    int n_add;
    const float* add[kMaxAdd]; int add_ctot[kMaxAdd], add_coff[kMaxAdd], add_shift[kMaxAdd];
    const float* zeros;        // >= 64 B of zeros in HBM: source for halo / padded-channel loads
    const float* w2; const float* bias2; float* out2; int out2_ctot, out2_coff, relu2;      // bf16 1x1 pair (layer1: Bottleneck k's 64 -> 256 expansion, then Bottleneck k+1's
                                                             // 256 -> 64 reduction from the tile the workgroup still holds in LDS): w2 packed [8][1][64][32], bias2 [64];
                                                             // out2: the reduction's NHWC bf16 view.  w2 == nullptr: none
    const float* in2; int in2_ctot, in2_coff, cin_split;     // bf16 1x1 only: input channels >= cin_split (a multiple of 32) come from a SECOND tensor of the same
                                                             // spatial size (a Bottleneck's last 1x1 and its 1x1 downsample as ONE GEMM over [t ; x]); in2 == nullptr: one input
    // filled by the launcher
    int R, G, Rin, Wp, PSTR, tiles_y, groups, TC, rows;
    float inv_RW, inv_Wo, inv_upc;   // 1 / (R*Wo), 1 / Wo, 1 / (PSTR/4) for the kernels' reciprocal-multiply divisions
    int nbuf;                  // bf16 kernel: patch buffers in LDS (2 = chunks double-buffered)
    int gx, gy, gx8, xcd;           // pixel tiles x output-channel blocks of the 1-D grid; xcd: XCD-aware block order (see xcd_block)
    int pw_stream;             // bf16 1x1 layers: 0 = never the stream kernel (conv_bf16_pw_stream), 1 = from the call size it pays at, 2 = whatever the call size
    int dbg;                   // timing-only ablation bits (tools/conv_micro.py); 0 in the product path
    int prio;                  // Winograd kernel: 0 = default wave priority, 1 / 2 = s_setprio 1 / 3 (critical-chain layers)
    int blk0, wsplit;          // Winograd kernel: first tile id of this launch; 1 = the 32-channel kernel on HALF a 64-channel block
                               // of weights packed for the 64-channel kernel (the half-size workgroups of a layer's last round)
};

// Returns hipSuccess or the launch error.  `tile_hint`: 0 = auto, 7 / 14 = force pixel sub-tiles.
hipError_t launch_conv(ConvArgs a, hipStream_t s, int tile_hint = 0);
// The configuration launch_conv runs: family 0 = whole-K tiles (conv_mfma_f32), 1 = split-K (conv_splitk_f32); tps = pixel tile / 16, tcs = channel
// tile / 16, nw = split-K waves (Cfg::nw), waves = waves per workgroup, width_variant = the image width of the edge-pointer split-K variant (0: generic),
// rows = output rows per tile
struct ConvChoice { int family = 0, tps = 0, tcs = 0, nw = 0, waves = 0, width_variant = 0, rows = 0; };
hipError_t conv_choose(const ConvArgs& a, int tile_hint, ConvChoice* out);
int conv_pick_tc(int Cout);                 // cout tile (32 or 64) -> defines CoutPad at pack time
hipError_t conv_init();                     // sets max dynamic LDS on every instantiation
const char* conv_dominant_kernel_name();

// ---- Winograd F(4x4,3x3) on the fp32 matrix cores for the 3x3 stride-1 layers on 56x56 / 28x28 maps (conv_wino4.hip): 2.25 multiplies per output
bool conv_wino4_eligible(int cin, int cout, int ks, int stride, int h, int w, int n_add);
hipError_t launch_conv_wino4(ConvArgs a, hipStream_t s, int* n_launches = nullptr);     // a.w = transformed weights [36][CinPad][CoutPad]
void pack_wino4_weights(const double* w_folded /* (cout,cin,3,3) */, int cout, int cin, int cin_pad, int cout_pad, float* out, int map_width = 56);
int conv_wino4_blocks(int cout, int map_width);   // 16-channel blocks per workgroup of that layer (4 or 2)
int conv_wino4_wide(int cout, int map_width);     // > 0: the layer runs conv_wino4w_f32 (eight waves) with that many 16-channel blocks per wave (4: 128 output channels per
                                                  // workgroup, 2: 64); weights packed as for 4 blocks
// What launch_conv_wino4 launches for `a` (a.N frames): waves per workgroup (4 / 8), nb (4-wave) or npw (8-wave) 16-channel blocks, the grid gx x gy,
// XCD-aware order, and split = 1: `full` workgroups of the 4-wave kernel, then the last `rest` as 2 * rest half-size ones
struct Wino4Form { int waves = 0, nb = 0, npw = 0, gx = 0, gy = 0, xcd = 0, split = 0, full = 0, rest = 0; };
hipError_t conv_wino4_form(const ConvArgs& a, Wino4Form* f);

void wino4_transform_filter(const double* g33, double* u36);   // U = G g G^T of F(4x4,3x3) in fp64
// ---- register-resident F(4x4,3x3) for the small maps (conv_wino4s.hip): 128 -> 128 @14x14, 256 -> 256 @7x7 (HR branches 2, 3), 256 -> 256 @14x14
// ---- layer1's 1x1 convolutions (64 -> 64 / 256, 256 -> 64 on 56x56 maps) with both operands straight from global memory (conv_pw.hip)
bool conv_pw_eligible(int cin, int cout, int ks, int stride, int h, int w, int n_add);
hipError_t launch_conv_pw(ConvArgs a, hipStream_t s);                     // a.w = the direct kernels' packing
// ---- the stem's first convolution (3 -> 64, 3x3, stride 2) with K = (channel, tap) flattened to 7 k-steps (conv_stem.hip)
bool conv_stem_eligible(int cin, int cout, int ks, int stride, int h, int w, int n_add);
hipError_t launch_conv_stem(ConvArgs a, hipStream_t s);                   // a.w = pack_stem_weights
void pack_stem_weights(const double* w_folded /* (64,3,3,3) */, float* out /* 7*4*64 */);
bool conv_wino4s_eligible(int cin, int cout, int ks, int stride, int h, int w, int n_add);
hipError_t launch_conv_wino4s(ConvArgs a, hipStream_t s, int ksplit);      // a.w = pack_wino4r_weights; ksplit 0: the shape's default
int conv_wino4s_images_per_tile(int map_width);                             // images per MFMA row tile (7x7: 4, 14x14: 1)
int conv_wino4s_row_tiles(int map_width, int n_images, int* last_tile_images);   // row tiles (workgroups per channel block) of a
                                                                                 // launch of n_images; *last_tile_images: images in the last one
void pack_wino4r_weights(const double* w_folded /* (cout,cin,3,3) */, int cout, int cin, float* out /* 36*cin*cout */);
// out = relu?( sum_k nearest_up(add_k) ), 1..4 addends, out and every addend are Views.
struct SumArgs {
    float* out; int out_ctot, out_coff;
    int N, C, H, W, relu, n_add;
    const float* add[4]; int add_ctot[4], add_coff[4], add_shift[4];
};
hipError_t launch_fuse_sum(const SumArgs& a, hipStream_t s);

// The up half of an HR module's fuse layer in one launch (hr_fuse.hip; hrnet.py:249-267, fuse layers hrnet.py:189-244):
// out_i = act(x_i + bias_i + sum_{j > i} nearest_up(W_ij . x_j) + sum_k extra_k) for outputs i = 0 .. nb-2 of a module with nb
// branches (branch b: 32 << b channels on a (56 >> b)^2 map); extra_k: the finished stride-2 chains D_ij, j < i (same shape as out_i).
struct FuseUpSrc { const float* x; int ctot, coff; const float* w; };      // x_j as a View, W_ij packed by pack_fuse_up_weights
struct FuseUpOut {
    float* out; int out_ctot, out_coff;
    const float* base; int base_ctot, base_coff;     // x_i
    const float* bias;                               // sum over j of the folded BatchNorm shifts, [32 << i]
    int relu, n_extra;
    const float* extra[2]; int extra_ctot[2], extra_coff[2];
    FuseUpSrc src[3];                                // j = i+1 .. nb-1
};
struct FuseUpArgs { int N, nb; FuseUpOut o[3]; int only = -1; };      // only >= 0 (bf16 launch): this output alone, grid N * 7
hipError_t launch_hr_fuse_up(const FuseUpArgs& a, hipStream_t s);
void pack_fuse_up_weights(const double* w_folded /* (cout, cin) */, int cout, int cin, float* out /* cout * cin */);
// the same launch on NHWC bf16 tensors (pointers address bf16 data, bias fp32); weights [cin / 32][cout][32] bf16
hipError_t launch_hr_fuse_up_bf16(const FuseUpArgs& a, hipStream_t s);
void pack_fuse_up_weights_bf16(const double* w_folded /* (cout, cin) */, int cout, int cin, unsigned short* out /* cout * cin */);

// nn.Upsample(scale_factor=2, mode='bilinear', align_corners=True) (hrnet.py:443)
hipError_t launch_bilinear2x(const float* in, float* out, int N, int C, int H, int W, hipStream_t s);

// crop + normalise: uint8 HWC frames (n,H,W,3) [or one shared frame] + boxes (n,4) -> (n,3,224,224) f32 (img_utils.py:252-285,355-363)
hipError_t launch_crop_normalise(const unsigned char* img, int H, int W, int per_image, const float* bbox, float scale, int bgr,
                                 float* out, int N, hipStream_t s);

// the same with OpenCV's fixed-point warpAffine arithmetic; maps: (N,mstride) doubles -- mstride 6: the inverse affine map of each frame;
// mstride 10: + iw, ih, tx, ty of the two-warp crop of a non-square box (iw = 0: one warp)
hipError_t launch_crop_normalise_cv(const unsigned char* img, int H, int W, int per_image, const double* maps, int mstride, int bgr, float* out, int N,
                                    hipStream_t s);

// PARE head tail ---------------------------------------------------------------------------
// softmax over H*W of heat[:,1+j] and attention pooling of feat channels (keypoint_attention.py:42-48)
// heat: (N,25,P) with channel 0 = background; featA (N,CA,P) -> outA (N,CA,24); featB (N,CB,P) -> outB (N,CB,24)
hipError_t launch_softmax_pool(const float* heat, int heat_ctot, const float* featA, int CA, const float* featB, int CB,
                               float* outA, float* outB, float* prob_ws, int N, int P, hipStream_t s);

struct TailWeights {
    const float* pose_w;    // (128,24,6): head.pose_mlp.weight (1,6,128,24,1,1) re-ordered at load so a channel's 144 weights are contiguous
    const float* shape_w;   // (10,1536)
    const float* shape_b;
    const float* cam_w;     // (3,1536)
    const float* cam_b;
};
// plf (N,128,24), csf (N,64,24) -> rot6d (N,24,6), shape (N,10), cam (N,3), rotmat (N,24,9), theta (N,85)
// pool_ws: the workspace launch_softmax_pool filled (per-range partial sums); plf / csf are WRITTEN here
hipError_t launch_head_tail(const float* pool_ws, bool range_stats /* per-range (max, sum) pairs in front of the partials: the softmax is finished here (both paths) */, float* plf, float* csf, TailWeights w, float* rot6d, float* shape, float* cam,
                            float* rotmat, float* theta, int N, hipStream_t s);
// the same tail from given features (second head pass of the use_gait_feat branch, grnet.py:165; plf / csf are inputs)
hipError_t launch_head_tail_from_feats(const float* plf, const float* csf, TailWeights w, float* rot6d, float* shape, float* cam, float* rotmat,
                                       float* theta, int N, hipStream_t s);
hipError_t launch_rot6d_to_rotmat(const float* x, float* R, int m, hipStream_t s);      // geometry.py:395-410
hipError_t launch_rotmat_to_aa(const float* R, float* aa, int m, hipStream_t s);        // geometry.py:68-97,159-293
size_t softmax_pool_ws_floats(int N);
constexpr int kPoolStatsFloats = 7 * 24 * 2;    // per frame, in front of the partial sums: [range][joint][max, sum of exp]
constexpr int kPoolSplit = 7;                 // pixel ranges of the attention pooling (3136 = 7 x 448): ONE constant for the fp32 and bf16 paths

constexpr int kBlendK = 220;       // rows of the blend-shape table: 207 pose + 10 shape + 1 template + 2 of padding (k-steps of 4)
constexpr int kSmplWsFloatsPerFrame = 288 + kBlendK;   // skinning matrices + the frame's row of the blend-shape GEMM
struct SmplTables {
    const float* blend;        // (220,20670) = [posedirs ; shapedirs^T ; v_template ; 0 0], assembled at load
    const int* skin_idx;       // (6890,skin_k) joints with a non-zero skinning weight, ascending, padded with -1
    const float* skin_w;       // (6890,skin_k)
    int skin_k;                // max non-zero weights per vertex (4 for a real SMPL model)
    const float* J_template;   // (24,3)   = J_regressor . v_template           (precomputed at load)
    const float* J_shapedirs;  // (24*3,10) = J_regressor . shapedirs             (precomputed at load)
    const float* lbs_weights;  // (6890,24)
    const int* thorax_idx;     // non-zero entries of row 5 ('Thorax (MPII)') of J_regressor_extra (9,6890): vertex ids ...
    const float* thorax_w;     // ... and weights
    int thorax_n;
    const int* parents;        // (24)
    int extra_ptr[10];         // all 9 rows of J_regressor_extra as one (vertex, weight) list: row r is entries extra_ptr[r] .. extra_ptr[r+1]-1,
    const int* extra_idx;      // vertex ids ascending within a row (csrc/smooth_kernels.hip; the thorax list above stays what launch_smpl reads)
    const float* extra_w;
};
// betas (N,10), rotmat (N,24,9), cam (N,3) -> verts (N,6890,3), kp3d (N,29,3), kp2d (N,29,2)
hipError_t launch_smpl(const float* betas, const float* rotmat, const float* cam, SmplTables t, float* A_ws,
                       float* verts, float* kp3d, float* kp2d, int N, hipStream_t s);

// The --smooth step (smooth_pose.py:28-116; csrc/smooth_kernels.hip, compiled without fma contraction) ----
constexpr int kOneEuroBlock = 32;  // frames per LDS staging block of the filter
struct OneEuroCoef { float a_d, one_minus_a_d, two_pi, min_cutoff, beta; };     // float32 constants of the recurrence, rounded once on the host
// x (T,72) with row stride ld >= 72 -> xhat (T,72): one workgroup, one sequence
hipError_t launch_one_euro(const float* x, int ld, int T, OneEuroCoef c, float* xhat, hipStream_t s);
// aa (m,3) -> R (m,3,3), smplx batch_rodrigues; betas_out != NULL: also betas_out (nb,10) = row betas0 (10) repeated (nb * 10 <= m)
hipError_t launch_aa_to_rotmat(const float* aa, float* R, int m, const float* betas0, float* betas_out, int nb, hipStream_t s);
int smooth_joint_count(int kind);  // 49 / 29 / 25 for GRNET_JOINTS_SPIN49 / _SPIN2 / _KINECTV2, 0: unknown
// kp29 (n,29,3) as launch_smpl wrote it (rows 0..23 are read), verts (n,6890,3) -> joints (n,smooth_joint_count(kind),3)
hipError_t launch_smpl_joints54(const float* kp29, const float* verts, SmplTables t, int kind, float* joints, int n, hipStream_t s);

// One box per sequence from 2D joints (batch_generation.py:39-93; csrc/bbox_kernels.hip, compiled without fma contraction) ----
constexpr int kBboxMaxJoints = 64;     // joints per frame: one wave lane each
constexpr int kBboxMaxFrames = 4096;   // frames per sequence: the heights of one sequence fit the LDS of the median's workgroup
constexpr double kBboxMinPixel = 500., kBboxSmallScale = 1.8;   // batch_generation.py:27-28 (MIN_PIXEL, BS)
constexpr int kMedoidRows = 256;       // rows per workgroup of the row-sum kernel, one per thread
constexpr int kMedoidTile = 1024;      // columns staged in LDS at a time (16 KiB)
constexpr int kMedoidMaxSplits = 64;   // column splits of one row tile
constexpr int kMedoidBatch = 128;      // sequences per launch: their offsets travel as a kernel argument
struct MedoidBatch { int n; int off[kMedoidBatch + 1]; };       // point offsets of n sequences lying back to back, from the start of the points
// columns of one split: the n columns in `splits` equal runs, rounded up to the row-sum kernel's unroll; split s covers [s c, min(n, (s + 1) c))
__host__ __device__ inline int medoid_split_columns(int n, int splits) { return ((n + splits - 1) / splits + 7) & ~7; }
// joints (frames,K,3) float64 -> points (frames K,4) float32 (x, y, s, 0) after the score rule, hgt (frames) float64
hipError_t launch_bbox_prepare(const double* joints, int K, int frames, double threshold, float* points, double* hgt, hipStream_t s);
// partial [splits][n] float64 per sequence, sequence q at partial + splits * off[q]: the sums of row i over the columns of each split
hipError_t launch_medoid_rowsum(const float* points, const MedoidBatch& b, int splits, double* partial, hipStream_t s);
// per sequence q of the batch (entry seq0 + q of the outputs; each may be NULL): the row of least cost, that cost, its (x, y)
hipError_t launch_medoid_argmin(const float* points, const MedoidBatch& b, int seq0, int splits, const double* partial, int* index, double* cost,
                                float* centre, hipStream_t s);
// off / K are frame offsets into hgt; bbox (n_seq,4) float64 = [cx, cy, nw, nh]
hipError_t launch_bbox_assemble(const double* hgt, const MedoidBatch& b, int seq0, int K, const float* centre, double* bbox, hipStream_t s);

// Pose metrics: MPJPE, PA-MPJPE, PVE, acceleration and acceleration error (csrc/metric_kernels.hip, compiled without fma contraction) ----
constexpr int kMetricMaxJoints = 64;   // joints per frame, selected joints and root joints: one wave lane each
constexpr int kMetricBatch = 128;      // sequences per launch: their offsets travel as a kernel argument
struct MetricBatch { int n; int off[kMetricBatch + 1]; };       // frame offsets of n sequences lying back to back, from the start of the call
struct MetricJoints { int n_select, n_root; unsigned char select[kMetricMaxJoints], root[kMetricMaxJoints]; };   // indices into the J joints
// per_frame (frames,5) float64 = [mpjpe, pa_mpjpe, pve, accel, accel_err] x unit: the joints launch writes columns 0, 1 and NaN into 3, 4 (and 2
// without vertices), the vertices launch column 2, the acceleration launch columns 3, 4 of the interior frames; transform (frames,13) or NULL
hipError_t launch_metric_joints(const float* pred, const float* gt, int J, int frames, const MetricJoints& mj, double unit, int has_verts, double* per_frame,
                                double* transform, hipStream_t s);
hipError_t launch_metric_accel(const float* pred, const float* gt, int J, const MetricBatch& b, const MetricJoints& mj, double unit, double* per_frame,
                               hipStream_t s);
hipError_t launch_metric_verts(const float* pred, const float* gt, int V, int frames, double unit, double* per_frame, hipStream_t s);
// seq_sum / seq_cnt (n_seq,5): the sums and counts of the structurally defined entries of sequence seq0 + q; per_seq (n_seq,5) or NULL: their means
hipError_t launch_metric_seq_means(const double* per_frame, const MetricBatch& b, int seq0, int has_verts, double* seq_sum, long long* seq_cnt,
                                   double* per_seq, hipStream_t s);
hipError_t launch_metric_total(const double* seq_sum, const long long* seq_cnt, int n_seq, double* total, hipStream_t s);
// K (k,9) float64 -> R (k,9), sigma (k,3): procrustes3() of procrustes3.h, one thread per matrix
hipError_t launch_procrustes(const double* K, int k, double* R, double* sigma, hipStream_t s);

// Camera-space trajectory: the translation fitted to 2D joints per frame, filled and summed up per sequence (csrc/translation_kernels.hip, compiled
// without fma contraction; the arithmetic: csrc/translation3.h) ----
constexpr int kTransMaxPairs = 64;     // (3D joint, 2D joint) pairs of the table
constexpr int kTransBatch = 64;        // sequences per launch: their offsets and intrinsics travel as a kernel argument
struct TransPairs { int n; int p3[kTransMaxPairs], p2[kTransMaxPairs]; };
struct TransBatch { int n; int off[kTransBatch + 1]; double cam[kTransBatch][3]; };      // frame offsets from the start of the call; (f, cx, cy) per sequence
// per_frame (frames,6) float64 = [tx, ty, tz, reproj_px, n_used, status]: one lane per frame
hipError_t launch_translation_fit(const float* joints3d, const float* joints2d, int K3, int K2, const TransPairs& pairs, const TransBatch& b, double threshold,
                                  int min_joints, double* per_frame, hipStream_t s);
// one workgroup per sequence: fills the unfitted rows of per_frame (fill != 0) and writes per_seq (n_seq,4) = [fitted, filled, mean reproj, path length]
// of sequence seq0 + q
hipError_t launch_translation_seq(const float* joints3d, int K3, int root, const TransBatch& b, int seq0, int fill, double* per_frame, double* per_seq,
                                  hipStream_t s);

// Per-frame boxes from 2D joints: tracked, gaps filled, smoothed (csrc/track_kernels.hip, compiled without fma contraction; the arithmetic:
// csrc/track_boxes.h) ----
constexpr int kTrackMaxJoints = 64;        // joints per frame
constexpr int kTrackMaxKernel = 31;        // the median's window, odd
constexpr double kTrackMaxSigma = 16.;     // the Gaussian's width: radius int(4 sigma + 0.5) <= 64, 129 weights
constexpr int kTrackMaxRadius = 64;
constexpr int kTrackMaxSeqs = 8192;        // sequences per call: their offsets and the weights travel through one pinned table
constexpr int kTrackThreads = 1024;        // threads of the sequence kernel's workgroup
constexpr int kTrackLdsFrames = 1024;      // frames of [start, end) whose median and Gaussian run in LDS (two buffers of three columns)
// params (frames,3) = [cx, cy, scale] of the detected frames (the others stay as they are); words: bit f & 63 of word f >> 6 = frame f detected,
// 4 * ceil(frames / 256) words
hipError_t launch_track_frames(const double* joints, int K, int frames, double vis_thresh, double* params, unsigned long long* words, hipStream_t s);
// one workgroup per sequence; off: n_seq + 1 frame offsets ON THE DEVICE; weights[0 .. radius] (radius < 0: no Gaussian), ksize 1: no median;
// work (frames,6); boxes (frames,4), status (frames), range (n_seq,2)
hipError_t launch_track_sequences(const int* off, int n_seq, const double* weights, int radius, int ksize, int pad, const double* params,
                                  const unsigned long long* words, double* work, double* boxes, int* status, int* range, hipStream_t s);
// the median (radius < 0) or the Gaussian alone on x, per sequence, into out (not x)
hipError_t launch_track_filter(const int* off, int n_seq, const double* x, const double* weights, int radius, int ksize, int pad, double* out, hipStream_t s);
// The Gaussian of the gait calls (sigma > 0 alone), a workgroup per (sequence, channel): column k of raw (channels,frames) inside each sequence into
// out[f * cols + col0 + k], the per-frame rows of the call (gait: cols 7, kinematics 13, contacts 4 from col0 1, regularity 4)
hipError_t launch_seq_gauss_columns(const int* off, int n_seq, int channels, const double* weights, int radius, int frames, const double* raw, double* out,
                                    int cols, int col0, hipStream_t s);

// Gait events and parameters from the 3D joints (csrc/gait_kernels.hip, compiled without fma contraction; the arithmetic: csrc/gait_events.h;
// DESIGN 4.11) ----
constexpr int kGaitMaxWindow = 32;         // frames on either side of an event
constexpr int kGaitThreads = 256;          // threads of the sequence kernel's workgroup: four waves, each a word of the event bitmasks at a time
constexpr int kGaitLdsWords = 64;          // words of each event bitmask a sequence keeps in LDS: 4096 frames (longer ones: the call's scratch)
struct GaitTable { int j[8]; };            // pelvis, spine-shoulder, left hip, right hip, left ankle, right ankle, left foot, right foot
// words of ONE bitmask of a call in its scratch, for the sequences too long for the LDS; a set of them is one mask over all sequences
inline size_t gait_mask_words(int frames, int n_seq) { return (size_t)(frames >> 6) + (size_t)n_seq + 1; }
inline size_t gait_mask_bytes(size_t sets, size_t mask_words) { return seq_args::align256(sets * mask_words * sizeof(unsigned long long)); }
// Where sequence q (frames f0 onwards) begins in a set of `words`.  Its ceil(T / 64) words end at or before (f1 >> 6) + q + 1, where the next sequence's
// begin: ceil(T / 64) <= (f1 >> 6) - (f0 >> 6) + 1.  So no two sequences overlap, and the last ends inside gait_mask_words.
__device__ __forceinline__ unsigned long long* gait_mask_at(unsigned long long* words, int f0, int q) { return words + (size_t)(f0 >> 6) + q; }
// per_frame (frames,7): column 4 (the width) always; columns 0 .. 3 (the signals) where raw is null, else raw (4,frames) gets them, a column each
hipError_t launch_gait_frames(const float* joints, int J, int frames, const GaitTable& tab, double* raw, double* per_frame, hipStream_t s);
// one workgroup per sequence, off: n_seq + 1 frame offsets ON THE DEVICE: events (frames), columns 5 and 6 of per_frame, per_seq (n_seq,18); words:
// 4 * mask_words; trans (frames,3) or null
hipError_t launch_gait_sequences(const int* off, int n_seq, int J, int pelvis, const float* joints, const double* trans, double fps, int window,
                                 double min_excursion, unsigned long long* words, size_t mask_words, double* per_frame, int* events, double* per_seq, hipStream_t s);
// the events rule alone on signals (frames,4) = [hL, hR, tL, tR]
hipError_t launch_gait_events(const int* off, int n_seq, const double* signals, int window, double min_excursion, int* events, hipStream_t s);

// Joint-angle kinematics per gait cycle (csrc/gait_kinematics_kernels.hip, compiled without fma contraction; the arithmetic: csrc/gait_angles.h;
// DESIGN 4.12) ----
constexpr int kKinMaxStride = 4096;        // frames between the two heel strikes of a stride
constexpr int kKinThreads = 256;           // threads of the cycle kernel's workgroup: four waves; threads 0 .. 100 own a cycle point each
constexpr int kKinLdsWords = 16;           // words of each heel-strike bitmask a sequence keeps in LDS: 1024 frames (longer ones: the call's scratch)
constexpr int kKinMaskSets = 26;           // bitmasks of a call in the scratch: left and right for each of the 13 channels' workgroups
struct KinTable { int j[16]; };            // pelvis, spine-shoulder, then left and right hip, knee, ankle, foot, shoulder, elbow, wrist
// per_frame (frames,13) where raw is null, else raw (13,frames) gets the angles, a column each
hipError_t launch_kin_frames(const float* joints, int J, int frames, const KinTable& tab, double* raw, double* per_frame, hipStream_t s);
// one workgroup per (sequence, channel): curves (n_seq,13,101,2), per_seq (n_seq,13,6); words: kKinMaskSets * mask_words (gait_mask_words)
hipError_t launch_kin_cycles(const int* off, int n_seq, const int* events, const double* per_frame, int min_stride, int max_stride, unsigned long long* words,
                             size_t mask_words, double* curves, double* per_seq, hipStream_t s);

// Turns and straight-walking gait parameters (csrc/gait_turns_kernels.hip, compiled without fma contraction; the arithmetic: csrc/gait_turns.h;
// DESIGN 4.13) ----
struct TurnRule;                           // gait_turns.h: fps and the thresholds of rule 4
// one workgroup per sequence: per_frame (frames,2) = [yaw step, yaw rate]; radius < 0: no Gaussian and raw is not used, else raw (frames) gets the raw
// rates; off: n_seq + 1 frame offsets ON THE DEVICE; tab: its first four joints are read
hipError_t launch_turn_rates(const int* off, int n_seq, const double* weights, int radius, int J, const GaitTable& tab, const float* joints, double fps,
                             double* raw, double* per_frame, hipStream_t s);
// one workgroup per sequence on per_frame (frames,2), the gait call's events (frames) and rows (frames,7): phase (frames), turns
// (n_seq,max_turns,7), per_seq (n_seq,24); words: kTurnMaskSets (gait_turns.h) * mask_words (gait_mask_words)
hipError_t launch_turn_sequences(const int* off, int n_seq, const TurnRule& rule, const double* per_frame, const int* events, const double* gait_rows,
                                 unsigned long long* words, size_t mask_words, int* phase, double* turns, double* per_seq, hipStream_t s);

// Foot contact phases and double support (csrc/gait_contacts_kernels.hip, compiled without fma contraction; the arithmetic: csrc/gait_contacts.h;
// DESIGN 4.14) ----
struct ContactRule;                        // gait_contacts.h: fps, the threshold's fraction or speed, the attribution's reach and limits
// one lane per frame: per_frame (frames,4) = [s, d_x, d_y, d_z]; raw null: no Gaussian follows and s is made here, else raw (3,frames) gets the
// vectors and per_frame is not written; off: n_seq + 1 frame offsets ON THE DEVICE; tab: its ankles (entries 4 and 5) are read
hipError_t launch_contact_frames(const int* off, int n_seq, const float* joints, int J, int frames, const GaitTable& tab, double fps, double* raw,
                                 double* per_frame, hipStream_t s);
// one workgroup per sequence on per_frame (frames,4) -- make_s: s is made from its smoothed vectors first -- or, per_frame null, on speeds (frames), and
// on the gait call's events (frames): phase (frames), runs (n_seq,max_runs,6), per_seq (n_seq,20); words: (kContactMaskSets + 1) (gait_contacts.h) *
// mask_words (gait_mask_words), the last set holding the block sums
hipError_t launch_contact_sequences(const int* off, int n_seq, const ContactRule& rule, double* per_frame, const double* speeds, bool make_s, const int* events,
                                    unsigned long long* words, size_t mask_words, int* phase, double* runs, double* per_seq, hipStream_t s);

// Gait regularity and symmetry from the autocorrelation of four body signals (csrc/gait_regularity_kernels.hip, compiled without fma contraction; the
// arithmetic: csrc/gait_regularity.h) ----
struct RegRule;                            // gait_regularity.h: fps, max_lag, min_lag, min_peak, min_pairs
constexpr int kRegLdsFrames = 64 * kGaitLdsWords;      // frames of a sequence whose centred signal and run numbers the sequence kernel keeps in LDS: 4096
// one lane per frame: the four signals into per_frame (frames,4), or, raw not null (a Gaussian follows), into raw (4,frames); trans (frames,3) or null
hipError_t launch_reg_frames(const float* joints, int J, int frames, const GaitTable& tab, const double* trans, double* raw, double* per_frame, hipStream_t s);
// a workgroup per (sequence, channel) on rows (frames,4) and exclude (frames) or null: acf (n_seq,4,max_lag+1), per_seq (n_seq,4,10).  Where a sequence
// has more than kRegLdsFrames frames: long_d (4,frames) float64, long_key (4,frames) int32 and words: 8 * mask_words (gait_mask_words); else null
hipError_t launch_reg_sequences(const int* off, int n_seq, const RegRule& rule, const double* rows, const int* exclude, int frames, double* long_d, int* long_key,
                                unsigned long long* words, size_t mask_words, double* acf, double* per_seq, hipStream_t s);

// Harmonic ratios per stride of the same four signals (csrc/gait_harmonics_kernels.hip, compiled without fma contraction; the arithmetic:
// csrc/gait_harmonics.h).  The frame kernel is launch_reg_frames ----
struct HarRule;                            // gait_harmonics.h: fps, n_harmonics, derivative, min_stride, max_stride, max_strides
// a workgroup per (sequence, channel) on rows (frames,4), the gait call's events (frames) and exclude (frames) or null: strides
// (n_seq,4,max_strides,6), spectrum (n_seq,4,n_harmonics,2), per_seq (n_seq,4,12).  slots: 4 * har_slots(frames, n_seq) of n_harmonics + 4 float64.
// Where a sequence has more than 64 * kGaitLdsWords frames: words: 8 * mask_words (gait_mask_words); else null
hipError_t launch_har_sequences(const int* off, int n_seq, const HarRule& rule, const double* rows, const int* events, const int* exclude, int frames,
                                unsigned long long* words, size_t mask_words, double* slots, double* strides, double* spectrum, double* per_seq, hipStream_t s);

// Sample entropy of the same four signals at several scales (csrc/gait_entropy_kernels.hip, compiled without fma contraction; the arithmetic:
// csrc/gait_entropy.h).  The frame kernel is launch_reg_frames ----
struct EntRule;                            // gait_entropy.h: m, fraction, derivative, scales
// two launches on rows (frames,4) and exclude (frames) or null: a workgroup per (sequence, channel) makes y (4,frames), the differenced signal, and
// per_seq (n_seq,4,4); a workgroup per (sequence, channel, scale) counts (n_seq,4,scales,3) int64.  z_long: (4 * scales,frames) float64 where a
// sequence has more than kRegLdsFrames frames, else null
hipError_t launch_ent_sequences(const int* off, int n_seq, const EntRule& rule, const double* rows, const int* exclude, int frames, double* y, double* z_long,
                                long long* counts, double* per_seq, hipStream_t s);

// Local dynamic stability of the same four signals (csrc/gait_stability_kernels.hip, compiled without fma contraction; the arithmetic:
// csrc/gait_stability.h).  The frame kernel is launch_reg_frames ----
struct StabRule;                           // gait_stability.h: derivative, dim, lag, theiler, horizon
// two launches on rows (frames,4) and exclude (frames) or null: a workgroup per (sequence, channel, block of kGaitThreads reference points, the blocks
// sized by `longest`, the call's longest sequence) finds nn (frames,4) int32; a workgroup per (sequence, channel) walks them into pairs
// (n_seq,4,horizon+1,2) int64 and mant (n_seq,4,horizon+1).  y_long: (4,frames) float64 where a sequence has more than kRegLdsFrames frames, else null
hipError_t launch_stab_sequences(const int* off, int n_seq, int longest, const StabRule& rule, const double* rows, const int* exclude, int frames, int* nn,
                                 double* y_long, long long* pairs, double* mant, hipStream_t s);

// Welch power spectral density of the same four signals (csrc/gait_spectrum_kernels.hip, compiled without fma contraction; the arithmetic:
// csrc/gait_spectrum.h).  The frame kernel is launch_reg_frames ----
struct SpecRule;                           // gait_spectrum.h: fps, derivative, segment, hop, nfft, f_lo, f_hi, min_segments
constexpr int kSpecThreads = 64;           // one wave per (sequence, channel, block of 64 bins): a lane owns a bin
constexpr int kSpecLdsSegments = 512;      // segments of a sequence whose starts and means the workgroup keeps in LDS (more: the call's scratch)
int spec_bin_blocks(int nfft);             // the grid's z: blocks of kSpecThreads bins among nfft / 2 + 1
// two launches on rows (frames,4) and exclude (frames) or null: a wave per (sequence, channel, block of bins) makes psd (n_seq,4,nfft/2+1) and the
// first three columns of per_seq (n_seq,4,13); a wave per (sequence, channel) the other ten.  y_long: (spec_bin_blocks * 4,frames) float64 where a
// sequence has more than kRegLdsFrames frames, else null; start_long int32 and mu_long float64 of that shape where a sequence can hold more than
// kSpecLdsSegments segments (spec_run_segments of its length), else null
hipError_t launch_spec_sequences(const int* off, int n_seq, const SpecRule& rule, const double* rows, const int* exclude, int frames, double* y_long, int* start_long,
                                 double* mu_long, double* psd, double* per_seq, hipStream_t s);

// Movement smoothness of the same four signals: spectral arc length and dimensionless jerk per segment (csrc/gait_smoothness_kernels.hip, compiled
// without fma contraction; the arithmetic: csrc/gait_smoothness.h).  The frame kernel is launch_reg_frames ----
struct SmoRule;                            // gait_smoothness.h: fps, derivative, segment, hop, nfft, f_cut, amplitude, min_segments
constexpr int kSmoWave = 64;               // one wave per (sequence, channel) lays the segments, and one reads the sequence's row off them
constexpr int kSmoThreads = 256;           // one workgroup per (slot, channel): a lane owns a bin, in rounds of this width
size_t smo_lds_bytes(const SmoRule& rule, int kc, int form);      // the segment kernel's dynamic LDS
// three launches (two where slots is 0) on rows (frames,4) and exclude (frames) or null: a wave per (sequence, channel) writes `start` of every slot
// of per_seg (slots,4,8), NaN behind the candidates, the first three columns of per_seq (n_seq,4,10) and, as scratch, tw (2 nfft float64: sine and
// cosine of har_twiddle(j, nfft)), slot_seq (slots) and slot_base (n_seq) int32; a workgroup per (slot, channel) the other seven columns of its row;
// a wave per (sequence, channel) the other seven of per_seq.  kc: smo_cut_bin(rule).  form: where the segment kernel reads its twiddles (0: tw)
hipError_t launch_smo_sequences(const int* off, int n_seq, int slots, const SmoRule& rule, int kc, int form, const double* rows, const int* exclude, double* tw,
                                int* slot_seq, int* slot_base, double* per_seg, double* per_seq, hipStream_t s);

// Arm swing and inter-limb coordination: auto and cross spectra of the two shoulder and the two hip flexions (csrc/gait_coordination_kernels.hip,
// compiled without fma contraction; the arithmetic: csrc/gait_coordination.h).  The workgroup is gait_spectrum's wave of kSpecThreads ----
constexpr int kCoordLdsFrames = 1024;      // frames of a sequence whose four differenced columns the workgroup keeps in LDS (more: the call's scratch)
constexpr int kCoordLdsSegments = 128;     // segments of a sequence whose starts and four means each the workgroup keeps in LDS (more: the call's scratch)
// one lane per frame: arm_left, arm_right, leg_left, leg_right into per_frame (frames,4), or, raw not null (a Gaussian follows), into raw (4,frames)
hipError_t launch_coord_frames(const float* joints, int J, int frames, const KinTable& tab, double* raw, double* per_frame, hipStream_t s);
// two launches on rows (frames,4) and exclude (frames) or null: a wave per (sequence, block of bins) makes au (n_seq,4,nfft/2+1), cr
// (n_seq,6,nfft/2+1,2) and the first columns of limbs (n_seq,4,13) and pairs (n_seq,6,10); a wave per (sequence, row) the others.  y_long:
// (spec_bin_blocks * 4 * frames) float64 where a sequence has more than kCoordLdsFrames frames, else null; start_long (spec_bin_blocks * frames) int32
// and mu_long (spec_bin_blocks * 4 * frames) float64 where a sequence can hold more than kCoordLdsSegments segments, else null
hipError_t launch_coord_sequences(const int* off, int n_seq, const SpecRule& rule, const double* rows, const int* exclude, int frames, double* y_long, int* start_long,
                                  double* mu_long, double* au, double* cr, double* limbs, double* pairs, hipStream_t s);

// Footprints, centre of mass and margin of stability (csrc/gait_balance_kernels.hip, compiled without fma contraction; the arithmetic:
// csrc/gait_balance.h).  The sequence kernel's workgroup is the gait call's kGaitThreads ----
struct BalanceRule;                        // gait_balance.h: fps, gravity, window, settle, max_step, max_steps
struct BalanceSegments;                    // gait_balance.h: the segment table, at most 16 rows, a kernel argument
constexpr int kBalanceLdsStrikes = 1024;   // marks (frames with a heel strike) of a sequence whose list the workgroup keeps in LDS: 4 KB (more: the call's scratch)
constexpr int kBalanceMaskSets = 3;        // left and right heel strikes, and the marks in front of each word
// one lane per frame: rel (frames,9) = [c, c - left ankle, c - right ankle]; tab: its ankles (entries 4 and 5) are read
hipError_t launch_balance_frames(const float* joints, int J, int frames, const GaitTable& tab, const BalanceSegments& seg, double* rel, hipStream_t s);
// one workgroup per sequence on rel (frames,9) and the gait call's events (frames): steps (n_seq,max_steps,15), per_seq (n_seq,24); words:
// kBalanceMaskSets * mask_words (gait_mask_words), list (frames) int32 and pairs (frames,20) float64 of scratch, which launch_balance_path reads
hipError_t launch_balance_steps(const int* off, int n_seq, const BalanceRule& rule, const double* rel, const int* events, unsigned long long* words,
                                size_t mask_words, int* list, double* pairs, double* steps, double* per_seq, hipStream_t s);
// one lane per frame behind launch_balance_steps, on its words and pairs: per_frame (frames,8)
hipError_t launch_balance_path(const int* off, int n_seq, int frames, const double* rel, const unsigned long long* words, size_t mask_words,
                               const double* pairs, double* per_frame, hipStream_t s);
// launch_balance_frames with the caller's centre of mass com (frames,3) in place of the segment table: rel (frames,9) = [com, com - left ankle, com - right ankle]
hipError_t launch_balance_com_frames(const float* joints, int J, int frames, const GaitTable& tab, const double* com, double* rel, hipStream_t s);

// The gait call's per-step and per-stride tables and bootstrap intervals of a per-step table (csrc/gait_bootstrap_kernels.hip, compiled without fma
// contraction; the arithmetic and the generator: csrc/gait_bootstrap.h).  The table kernel's workgroup is the gait call's kGaitThreads
// and its LDS masks are kGaitLdsWords long ----
struct BootRule;                           // gait_bootstrap.h: the table's shape, the columns, B, block, seed, stream and the quantiles, a kernel argument
constexpr int kStepMaskSets = 3;           // left and right heel strikes, and the frames that are not straight
constexpr int kBootThreads = 1024;         // lanes of the bootstrap's workgroup: each takes the replicates lane, lane + 1024, ...
constexpr int kBootRounds = 5;             // replicates of a lane at most: 0 .. 4096 over 1024 lanes
// one workgroup per sequence on the gait call's events (frames) and rows (frames,7); phase (frames) or null (null: every step and stride is listed):
// steps (n_seq,max_rows,6), strides (n_seq,max_rows,4), counts (n_seq,2); words: kStepMaskSets * mask_words (gait_mask_words) of scratch
hipError_t launch_step_tables(const int* off, int n_seq, const int* events, const int* phase, const double* per_frame, double fps, int max_rows,
                              unsigned long long* words, size_t mask_words, double* steps, double* strides, int* counts, hipStream_t s);
// one workgroup per (sequence, column, statistic) on table (n_seq,max_rows,C) and counts (n_seq): out (n_seq,n_cols,3,2 + n_q), replicates (n_seq,n_cols,3,B) or null
hipError_t launch_bootstrap(const double* table, const int* counts, int n_seq, const BootRule& rule, double* out, double* replicates, hipStream_t s);

// Recurrence quantification of the same four signals (csrc/gait_recurrence_kernels.hip, compiled without fma contraction; the arithmetic:
// csrc/gait_recurrence.h).  The frame kernel is launch_reg_frames ----
struct RecRule;                            // gait_recurrence.h: derivative, dim, lag, theiler, radius
// gait_entropy's first launch alone (csrc/gait_entropy_kernels.hip): y (4,frames) and per_seq (n_seq,4,4) = (n, mu, SD, fraction SD)
hipError_t launch_ent_spread(const int* off, int n_seq, int derivative, double fraction, const double* rows, const int* exclude, int frames, double* y,
                             double* per_seq, hipStream_t s);
// three launches on rows (frames,4) and exclude (frames) or null: launch_ent_spread into y and spread (n_seq,4,4); a workgroup per (sequence, channel,
// part; max_parts: the most parts of a sequence, rec_parts) walks the pairs into partials (sum of the sequences' parts,4,kRecPartCols) int64; a
// workgroup per (sequence, channel) adds them into per_seq (n_seq,4,5), hist (n_seq,4,255) int64 and counts (n_seq,4,6) int64
hipError_t launch_rec_sequences(const int* off, int n_seq, int max_parts, const RecRule& rule, const double* rows, const int* exclude, int frames, double* y,
                                double* spread, long long* partials, double* per_seq, long long* hist, long long* counts, hipStream_t s);

// Joints regressed from vertices with a caller's table (pare.py:70-76; csrc/joint_regress.hip) ----
constexpr int kJregMaxRows = 64;   // output rows per frame (4 MFMA row tiles)
constexpr int kJregSlices = 27;    // fixed split of the 6890 vertices: 27 workgroup slices of 256 (4 waves x 64), partials added in slice order
constexpr int kJregChunks = 16;    // frame chunks per call = table reads per call (8: 24 us, 16: 19 us, 32: 21 us at 400 frames)
size_t joint_regress_pack_floats(int jout);
size_t joint_regress_workspace_floats(int jout, int max_frames);
void joint_regress_pack(const float* W /* (jout,6890) host */, int jout, float* out /* joint_regress_pack_floats(jout) host */);
// verts (n,6890,3), 8-byte aligned -> joints (n,jout,3); partial: joint_regress_workspace_floats(jout, >= n) device floats
hipError_t launch_joint_regress(const float* verts, const float* wpack, int jout, float* partial, float* joints, int n, hipStream_t s);

// The mesh overlay of demo.py --mesh_render (lib/utils/renderer.py:78-126; csrc/render_kernels.hip) ----
constexpr int kRasterSlots = 16;             // meshes per launch group: each has its own depth image and vertex records in the workspace
constexpr int kRasterMaxDim = 4096;          // largest image side
// kRasterSnapBits = 8, the sub-pixel bits of the snapped window coordinates: raster_lines.h
constexpr int kRasterCoordLimit = 1 << 28;   // |X|, |Y| are clamped here: coordinate differences < 2^29 + 2^21, edge products < 2^59, their sums fit int64
struct RasterView { float M[9]; int H, W; };                      // q = M (x, -y, -z); the viewport
struct RasterMesh {                                               // the topology of one mesh, device pointers (grnet_load_faces)
    const int* faces;      // (n_faces,3)
    const int* vf_off;     // (n_verts+1) row offsets of ...
    const int* vf_idx;     // ... the faces at each vertex, ascending face index
    int n_verts, n_faces;
};
struct RasterWork {                                               // per slot s: element s * n_verts of the vertex records, s * H * W of depth
    float* q;              // (slots,n_verts,3) transformed positions
    int* xy;               // (slots,n_verts,2) snapped window coordinates
    float* z;              // (slots,n_verts)   z_ndc
    float* nrm;            // (slots,n_verts,3) unit vertex normals in q space
    int* bbox;             // (slots,4) max over the vertices of (-X, -Y, X, Y)
    unsigned long long* depth;   // (slots,H,W) (ordered z << 32) | face, GL rows
};
struct RasterChunk {                                              // what the host knows about the meshes of one launch group
    int n;                          // <= kRasterSlots
    int mesh[kRasterSlots];         // index into verts / cams of the call
    int image[kRasterSlots];
    float colour[kRasterSlots][3];  // in the image's memory order
};
size_t raster_depth_words(int H, int W);     // 64-bit words of one depth image
// verts (n,n_verts,3), cams (n,4) -> the vertex records and the bounding box of every slot of the chunk (a memset and two launches)
hipError_t launch_raster_setup(const float* verts, const float* cams, const RasterChunk& c, const RasterView& v, const RasterMesh& m, RasterWork w, hipStream_t s);
// depth of every slot: cleared inside the mesh's bounding box, then the z-buffer over the faces (two launches)
hipError_t launch_raster_cover(const RasterChunk& c, const RasterView& v, const RasterMesh& m, RasterWork w, hipStream_t s);
// shade the covered pixels of every slot into its image: images (F,H,W,3) uint8, every other byte untouched
hipError_t launch_raster_resolve(const RasterChunk& c, const RasterView& v, const RasterMesh& m, RasterWork w, unsigned char* images, hipStream_t s);
// slot 0's winning face per pixel in IMAGE rows, -1 where uncovered: winner (H,W) int32, every element written
hipError_t launch_raster_winner(const RasterView& v, RasterWork w, int* winner, hipStream_t s);
// The wireframe (demo.py --mesh_render --wireframe): the three edges of every front face as 1-pixel lines; the low word of a depth key is
// 3 face + k, k = 0: v0 -> v1, 1: v1 -> v2, 2: v2 -> v0.  Same two launches each as the filled pair above; the depth clear and the resolve
// reach one pixel further than the fill's, to every pixel whose SQUARE meets the bounding box.
constexpr int kRasterLineWaveSteps = 16;     // an edge of more major steps than this is walked by the whole wave (unmeasured: NOTES_rejected)
hipError_t launch_raster_lines_cover(const RasterChunk& c, const RasterView& v, const RasterMesh& m, RasterWork w, hipStream_t s);
hipError_t launch_raster_lines_resolve(const RasterChunk& c, const RasterView& v, const RasterMesh& m, RasterWork w, unsigned char* images, hipStream_t s);
// the wireframe's depth clear alone, over `slots` depth images and their bounding boxes: the skeleton view's clear
hipError_t launch_raster_lines_clear(const RasterView& v, RasterWork w, int slots, hipStream_t s);

// Volume, centre of mass, central second moments and area of the closed mesh (csrc/mesh_moments_kernels.hip, compiled without fma contraction; the
// arithmetic: csrc/mesh_moments.h) ----
constexpr int kMeshFormDirect = 0, kMeshFormStaged = 1;     // the corners gathered from global memory / from a copy of the frame in LDS: the same bits
constexpr int kMeshFormDefault = kMeshFormDirect;           // the faster one on an MI355X (profiles/mesh_moments_times.txt)
// one workgroup per frame on verts (n,m.n_verts,3) and the table of m: rows (n,11), sums (n,11) or null
hipError_t launch_mesh_moments(const float* verts, int n, const RasterMesh& m, int form, double* rows, double* sums, hipStream_t s);

// The 3D skeleton view of demo.py --skeleton_view (demo.py:303-361, lib/utils/vis.py:571-587; csrc/skeleton_kernels.hip) ----
// Wide line segments between projected points, ALL skeletons aimed at an image in ONE depth image.  A launch group is up to kRasterSlots
// IMAGES, slot s with its own depth image and bounding box in RasterWork (q and nrm unused); the skeletons aimed at them go through in batches
// whose records are kernel arguments.
constexpr int kSegMaxPoints = 1024, kSegMaxSegments = 4096, kSegMaxWidth = 16;
constexpr int kSegBatchSkeletons = 64;       // skeletons per launch of the setup and of the cover: their records are a kernel argument (1 KiB)
constexpr int kSegGroupPoints = 65536;       // projected points (xy, depth) the workspace's record area holds at a time: 64 skeletons of 1024 points
constexpr int kSegWindowLimit = 1 << 20;     // a window coordinate beyond this many pixels makes a point invalid; snapped: kRasterCoordLimit
struct SegView {
    float R[9];                    // the body rotation, row-major, applied first
    float X[4], Y[4], Wh[4];       // x_win = cx + X.(p,1) / hw, y_win = cy + Y.(p,1) / hw, hw = Wh.(p,1): projection and window folded on the host in double
    float cx, cy;
    int H, W;
};
struct SegSegment { int a, b, width, colour; };   // point indices, pixels, the three bytes in memory order (byte k: bits 8k..8k+7)
struct SegSkeleton { int index, slot, rank, pad; };  // row of the call's points, the image's slot in the group, its rank among the skeletons of that image
struct SegBatch {                                 // the skeletons of one launch
    int n;                         // <= kSegBatchSkeletons
    int base;                      // skeleton k's points are records (base + k) * P ... of w.xy / w.z
    SegSkeleton rec[kSegBatchSkeletons];
};
struct SegGroup { int n; int image[kRasterSlots]; };
struct SegTables { const SegSegment* seg; int S, P; };
// points (n,P,3) -> w.xy / w.z of the batch's skeletons (INT_MIN in both coordinates: invalid) and the slots' bounding boxes grown by pad
hipError_t launch_segments_setup(const float* points, const SegView& v, SegTables t, const SegBatch& b, int pad, RasterWork w, hipStream_t s);
// one wave per (skeleton, segment): 64-bit atomicMin of (ordered(depth) << 32) | (rank S + segment) on every pixel of the wide line
hipError_t launch_segments_cover(const SegView& v, SegTables t, const SegBatch& b, RasterWork w, hipStream_t s);
// the colour of the winning segment into every covered pixel of the slots' bounding boxes: images (F,H,W,3) uint8, every other byte untouched
hipError_t launch_segments_resolve(const SegView& v, const SegGroup& g, SegTables t, RasterWork w, unsigned char* images, hipStream_t s);

// GRU gait encoder (gait_feat_encoder.py:79-104) ------------------------------------------------
struct GruWeights {
    const float* cparam_w;                 // (128,3,24)
    const float* w_ih[2][2]; const float* w_hh[2][2]; const float* b_ih[2][2]; const float* b_hh[2][2];  // [layer][dir]
    const float* speed_w0; const float* speed_b0; const float* speed_w2; const float* speed_b2;
    const float* step_w0;  const float* step_b0;  const float* step_w2;  const float* step_b2;
    const float* phase_w0; const float* phase_b0; const float* phase_w2; const float* phase_b2;
};
struct GruWorkspace {
    float* xin;      // (b*T, 3072)   x + xc
    float* gi;       // (2, b*T, 900) input projections per direction
    float* l0;       // (b*T, 600)
    float* l1;       // (b*T, 600)
    float* hfin;     // (b, 1200)
    int mode = 3;                         // GRNET_OPT_GRU_MODE: recurrence form 0 .. 3 (+ 16: agent-scope granule stores whatever the placement)
    unsigned* fault = nullptr;            // host-visible word the split kernels set when a hand-off poll ran into its bound (the results of that call are NaN-poisoned)
    unsigned long long* xbuf = nullptr;   // b * kGruXbufU64PerSeq 8-byte words: (b, 2 dirs, 2 parities, 300) {h value, step tag} granules of the split recurrence, then
                                          // (b, 2 dirs, 8 slices) {XCC id, 1} placement words (may be null: the unsplit kernel runs)
};
constexpr int kGruXbufU64PerSeq = 2 * 2 * 300 + 2 * 8;
// bf16 path, round 6 (conv_bf16_roll.hip): the stem pair and a whole layer1 Bottleneck as ONE launch, a workgroup walking a frame row by row
hipError_t conv_bf16_roll_init();
int conv_bf16_roll_segments(int n_frames);          // row segments per frame of those launches (1, 2 or 4: frames x segments >= CUs)
hipError_t launch_conv_bf16_bneck(const void* in, int in_ctot, int in_coff, void* out, int out_ctot, int out_coff, int N, bool first, const void* w1, const float* b1,
                                  const void* w2, const float* b2, const void* w3, const float* b3, hipStream_t s);
hipError_t launch_conv_bf16_stem_pair(const float* frames, void* out, int out_ctot, int out_coff, int N, const void* w1pk, const float* b1, const void* w2, const float* b2,
                                      hipStream_t s);
// bf16 path (conv_bf16.hip): NHWC bf16 activations, fp32 accumulation on the bf16 matrix cores ----------------------
hipError_t conv_bf16_init();
hipError_t launch_conv_bf16(ConvArgs a, hipStream_t s, int tile_hint = 0);     // pointers in `a` address bf16 data (bias fp32)
// A chain of BasicBlocks of one HR branch in ONE launch, the frame resident in LDS (conv_bf16_chain.hip): convolutions 2k, 2k+1 are conv1 / conv2 of
// block k (hrnet.py:43-59), every one C -> C, 3x3, stride 1, ReLU; conv2 adds the block's input.  (C, W) in {(64,28), (128,14), (256,7)}: ONE launch;
// (32,56): the whole chain as one pipeline of rows (conv_bf16_chain_pipe), or one launch per block, a workgroup walking the bands of a frame (conv_bf16_block_frame).
constexpr int kMaxChain = 8;
struct ChainArgs {
    const void* in; int in_ctot, in_coff;       // NHWC bf16 view (N, W, W, C)
    void* out; int out_ctot, out_coff;
    int N, nconv;
    const void* w[kMaxChain];                   // [C/32][9][C][32] bf16, BatchNorm folded
    const float* bias[kMaxChain];               // fp32 [C]
    void* mid[kMaxChain / 2 - 1];               // (32, 56) only -- one launch per BasicBlock: the output of block k < nconv/2 - 1
    int mid_ctot[kMaxChain / 2 - 1], mid_coff[kMaxChain / 2 - 1];
    int flags = 0;                                   // bit 0 (conv_bf16_block_frame): the block's output through the plane + 16-byte stores instead of straight from the accumulators (A/B)
};
int conv_bf16_chain_launches(int c, int w, int nconv);
hipError_t conv_bf16_chain_init();             // sets the dynamic LDS of the kernels of conv_bf16_chain.hip, then calls the two below
hipError_t conv_bf16_wide_init();
hipError_t conv_bf16_s2_init();
bool conv_bf16_chain_eligible(int c, int w);
hipError_t launch_conv_bf16_chain(const ChainArgs& a, int c, int w, hipStream_t s);
// one wide 3x3 stride-1 convolution with a band of the input resident in LDS (conv_bf16_wide.hip: conv_bf16_wide_band, conv_bf16_wide_ring); pointers as launch_conv_bf16
bool conv_bf16_wide_eligible(const ConvArgs& a);
hipError_t launch_conv_bf16_wide(const ConvArgs& a, hipStream_t s);
// one 3x3 stride-2 convolution with a band of the input resident in LDS, de-interleaved by row / column parity (conv_bf16_s2.hip: conv_bf16_s2_band, conv_bf16_s2_rows)
bool conv_bf16_s2_eligible(const ConvArgs& a);
hipError_t launch_conv_bf16_s2(const ConvArgs& a, hipStream_t s);
hipError_t launch_nchw_f32_to_nhwc_bf16(const float* in, void* out, int N, int C, int H, int W, int Cp, hipStream_t s);
// the stem's 3 -> 64 stride-2 convolution straight from the caller's fp32 NCHW frames (N,3,224,224) to NHWC bf16 (N,112,112,out_ctot)
hipError_t launch_conv_bf16_stem(const float* frames, const void* wpk, const float* bias, void* out, int out_ctot, int out_coff, int N, int relu, hipStream_t s);
void pack_stem_weights_bf16(const double* w_folded /* (64,3,3,3) */, unsigned short* out /* 4*64*8 */);
hipError_t launch_nhwc_bf16_to_nchw_f32(const void* in, float* out, int N, int C, int H, int W, int ctot, int coff, hipStream_t s);
hipError_t launch_bilinear2x_bf16(const void* in, void* out, int N, int C, int H, int W, hipStream_t s);
hipError_t launch_fuse_sum_bf16(const SumArgs& a, hipStream_t s);
hipError_t launch_softmax_pool_bf16(const void* heat, int hc, const void* featA, int CA, int ctA, const void* featB, int CB, int ctB, float* pool_ws, int N,
                                    int P, hipStream_t s);

// C[M][N] = A[M][K] . B[N][K]^T + bias[N] on the fp32 matrix cores (row-major, K % 4 == 0, 16-byte aligned rows).
// split-K partial sums of few-row GEMMs live in scratch lent by the caller (kGemmWsFloats floats are always enough: a GEMM only splits
// while M*N < 128 tiles of 64x64, and into at most 16 slices); without it the launcher falls back to hipMallocAsync.
constexpr size_t kGemmWsFloats = (size_t)16 * 128 * 4096;
void set_gemm_workspace(float* ws, size_t floats);
hipError_t launch_gemm_nt_bias(const float* A, const float* B, const float* bias, float* C, int M, int N, int K, int ldc, hipStream_t s);

// Temporal taps (grnet_temporal_taps): while a sink is installed on this thread, launch_gru / launch_tsattn / launch_featcorr / launch_gait_cparams enqueue a
// device-to-device copy of each stage's output right behind the launch that wrote it -- the temporal scratch cannot be read after the call (x_t is gated in place,
// yt | ys | x1 hold the key-part partials before their own values, the GRU's gi becomes the heads' hidden buffer).  The launches, their order, buffers and aliasing
// are the production ones; without a sink tap() is one pointer test and enqueues nothing.  `layout` gets one line per copy, "tap <name> <offset> <dims...>", and
// one per GEMM, "gemm <M> <N> <K> <splits>" (launch_gemm_nt_bias).
struct TapSink {
    float* buf = nullptr;
    size_t floats = 0, used = 0;
    std::string layout;
};
extern thread_local TapSink* g_taps;
hipError_t tap_copy(const char* name, const float* src, std::initializer_list<size_t> shape, hipStream_t s);
inline hipError_t tap(const char* name, const float* src, std::initializer_list<size_t> shape, hipStream_t s) {
    return g_taps ? tap_copy(name, src, shape, s) : hipSuccess;
}
size_t gru_tap_floats(int b, int T);
hipError_t tsattn_tap_floats(int b, int n, size_t* floats);
hipError_t featcorr_tap_floats(int b, int n, size_t* floats);      // launch_gait_cparams + launch_featcorr (the attention block included)

// TSAttnBlock (attention_utils.py:219-270) weights, reference layouts: Linear weights (out, in); jw1 (64,128,24), jw2 (128,64,24).
struct TsAttnWeights {
    const float *n1_g, *n1_b, *n2_g, *n2_b;
    const float *qkv_t_w, *qkv_t_b, *ts_w, *ts_b, *qkv_s_w, *qkv_s_b, *fc_s_w, *fc_s_b, *fc_t_w, *fc_t_b;
    const float *jw1, *jw2;
};
size_t tsattn_ws_floats(int b, int n);
// longest clip the temporal attention takes: its softmax row over the clip's frames lives in LDS ((512 + n) floats <= 160 KB)
constexpr int kTsAttnMaxFrames = 32768;
int tsattn_max_frames();        // min(kTsAttnMaxFrames, what the CURRENT device's LDS per workgroup holds): the up-front refusal matches the device
// x (b,n,3072) index c*24+j, xs (b,n,3200) index c*25+t -> y (b,n,3072); ws: tsattn_ws_floats(b, n) floats of scratch.
hipError_t launch_tsattn(const float* x, const float* xs, const TsAttnWeights& w, float* ws, float* y, int b, int n, hipStream_t s);
// what launch_tsattn does with a clip of n frames on the CURRENT device, from the functions it calls itself: plan[0] kernel (0 per-query, 1 blocked),
// plan[1] key parts per (query tile, head) (1: no combine launch), plan[2] key blocks of 32 (per-query: 0), plan[3] dynamic LDS bytes of the attention launch
hipError_t tsattn_plan(int n, int plan[4]);

// FeatCorrector (feature_correction.py:104-157) pieces around the GRU and the attention block; BatchNorm1d folded to scale / shift at load.
struct FeatCorrWeights {
    const float *t0_w, *t0_b, *t3_w, *t3_b;      // gfeat_mpl_t: (1536,7), (1536), (3072,1536), (3072)
    const float *s0_w, *s0_b, *s3_w, *s3_b;      // gfeat_mpl_s: (64,7), (64), (128,64), (128)
    const float *bn_scale, *bn_shift;            // bn_in   (3072)
    const float *bns_scale, *bns_shift;          // bn_in_s (3200)
};
size_t featcorr_ws_floats(int b, int n);
hipError_t launch_gait_cparams(const float* cam, int cam_ld, const float* bbox, const float* cimg, float* cparams, int M, hipStream_t s);
hipError_t launch_featcorr(const float* x, const float* avg, const float* phase, const FeatCorrWeights& w, const TsAttnWeights& tw, float* ws, float* out,
                           int b, int n, hipStream_t s);

hipError_t launch_gru(const float* x, const float* cparams, GruWeights w, GruWorkspace ws, float* y, float* phase,
                      float* xc, int b, int T, hipStream_t s);

}  // namespace grk
