/*
 * libgrnet_hip.so -- C ABI of the MI355X-native MAX-GRNet per-frame inference path.
 *
 * The reference has no FFI for this path: it sits behind a plain torch.nn.Module.  Each entry
 * point below names the reference interface it replaces (file:line under the reference repo);
 * INTEGRATION.md shows the ctypes binding a maintainer adds on the reference side.
 *
 * Conventions: every function returns 0 on success or a negative GRNET_E* code and never throws
 * across the ABI; grnet_last_error() returns a static-lifetime (per handle) message.  One handle
 * per GPU per process; a handle is not thread-safe (one caller thread + its stream); different
 * handles are independent.  All device work is enqueued on the stream passed in (a hipStream_t,
 * passed as void*); grnet_forward performs no allocation and no host synchronisation, so it can
 * be captured into a hipGraph by the caller (or by the library: GRNET_OPT_USE_GRAPH).
 * All tensors are fp32, dense, row-major ("C order"); device pointers are plain HIP device
 * pointers (e.g. torch.Tensor.data_ptr()), owned by the caller and never freed by the library.
 *
 * Environment.  The library reads exactly these variables (tests/test_host_cpu.py greps csrc/ for any other getenv):
 *   GRNET_TRACE=1        one line per plan / schedule / tuning decision on stderr; no effect on results
 *   GRNET_MULTI_LANE=0   process-wide default of GRNET_OPT_MULTI_LANE (profiling: the launches one after another on one stream)
 *   GRNET_WINO=0         process-wide default of GRNET_OPT_WINOGRAD
 *   GRNET_BF16_CHAIN=<mask>  process-wide default of GRNET_OPT_BF16_CHAIN
 *   GRNET_RCCL_LIB=<name>    the ONE library the exchange binds instead of librccl.so.1 (csrc/exchange.cpp)
 * The Python host adds GRNET_LIB_PATH (load another build of this library, tools/ only) and bench.py GRNET_BENCH_BACKEND (gloo rehearsals).
 * Every other GRNET_* name that earlier rounds' notes mention is an A/B switch of DIAGNOSTIC builds (make ABLATION=1; csrc/kernels.h
 * GRNET_AB): in this library it is a compile-time constant and setting the variable does nothing.
 */
#ifndef GRNET_HIP_H
#define GRNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct grnet grnet_t;

#define GRNET_OK 0
#define GRNET_EINVAL (-22)   /* bad argument / shape */
#define GRNET_ENOENT (-2)    /* missing weight tensor at finalize */
#define GRNET_ENOMEM (-12)
#define GRNET_EHIP (-5)      /* a HIP runtime call failed; see grnet_last_error */
#define GRNET_ESTATE (-1)    /* call order violated (e.g. forward before finalize) */

#define GRNET_DTYPE_F32 0
#define GRNET_DTYPE_I64 1    /* accepted for num_batches_tracked, ignored */

/* GRNet(...).to(device) -- lib/models/grnet.py:27-91, demo.py:106-111.  Allocates every
 * activation buffer for up to max_frames frames per call (the reference's batch axis N = B*T,
 * grnet.py:136-138).  dtype: 0 = fp32 (the reference's precision; the 1e-3 parity bar is stated for it);
 * 1 = bf16 storage (NHWC activations, folded weights) with fp32 accumulation on the bf16 matrix cores and an fp32 tail
 * (pooling sums, MLPs, SMPL) -- BASELINE configs 3 and 5; inputs and outputs of every entry point stay fp32. */
int grnet_create(grnet_t** out_handle, int device_id, int dtype, int max_frames);

/* The same constructor with named precisions and flags; grnet_create(out, dev, p, n) == grnet_create_ex(out, dev, p, n, 0).
 * GRNET_CREATE_COMPACT_ARENA: intermediate tensors whose lifetimes cannot overlap share memory: 13.7 MB per frame of
 * max_frames in fp32 (14.2 MB on a bf16 handle) against the 103.8 MB of the default layout, which gives every intermediate its own buffer.  A tensor may
 * lie under a later one only if every launch that reads or writes it is ordered before every launch that writes the later one by the
 * plan's OWN read-after-write dependencies, in every launch form (any call size, tuning table or GRNET_OPT_BF16_CHAIN mask): no launch,
 * event or wait is added or moved, and every output of every entry point is bit-identical to a default handle's.
 * What a compact handle cannot do: grnet_debug_tensor serves only tensors nothing is placed over later in the forward (cat and the views
 * that write it, head.heat, head.smpl_feats, head.cam_shape and whatever else the layout leaves last in its bytes -- a static property of
 * the layout, listed by grnet_arena_layout); every other name returns GRNET_ESTATE.  grnet_tune and grnet_time_conv work as before (they
 * leave garbage in the buffers on either kind of handle).
 * GRNET_EINVAL: an unknown flag or precision, max_frames outside [1, 2048]. */
#define GRNET_PRECISION_F32 0
#define GRNET_PRECISION_BF16 1
#define GRNET_CREATE_COMPACT_ARENA 1u
int grnet_create_ex(grnet_t** out_handle, int device_id, int precision, int max_frames, unsigned flags);

/* The activation arena of a handle that grnet_create_ex(precision, max_frames, flags) would make, computed on the host: no handle, no
 * device, no HIP call (a machine without a GPU can size a deployment, and the tests prove the layout there).
 * info[0] bytes this layout allocates, info[1] bytes the default (full) layout allocates, info[2] a lower bound for any layout under the
 * sharing rule -- the largest sum of tensors alive across one launch (written by it or before it, used by it or after it), over every op
 * and every launch group, plus the fixed blocks --, info[3] the number of tensors, info[4] how many of them share bytes with another.
 * All three sizes include the 256-byte zero block in front and the 256 bytes of tail. */
int grnet_arena_query(int precision, int max_frames, unsigned flags, int64_t* info /* 5 */);
/* The same layout as text, one line per item:
 *   tensor <id> <debug name or -> <floats per frame> <offset in floats from the arena's base>
 *   op <index> <kind> reads <tensor ids...> writes <tensor ids...>      the plan in the order it is written; the last one, COPYOUT, stands
 *                                                                       for the forward's copies of cat / head.heat / head.smpl_feats
 *   group <op indices...>                                               ops that some launch form runs as ONE launch (bf16 kernel groups)
 * A tensor occupies floats-per-frame x max_frames floats rounded up to 256 bytes (bf16 handles size their buffers in floats as well).
 * buf NULL: returns the bytes needed; else the length written, or GRNET_EINVAL if size is too small. */
int grnet_arena_layout(int precision, int max_frames, unsigned flags, char* buf, int size);
/* info[0..4] of grnet_arena_query for a live handle (equal to the query's for the handle's precision, max_frames and flags). */
int grnet_arena_info(grnet_t* h, int64_t* info /* 5 */);
/* Diagnostic: fills the whole arena behind the leading zero block with a 32-bit pattern (hipMemsetD32Async on `stream`).  A forward reads
 * nothing it did not write, so its outputs do not depend on the pattern (tests/test_gpu_compact_arena.py). */
int grnet_arena_fill(grnet_t* h, uint32_t pattern, void* stream);
/* The assignment itself, on any conflict graph: n buffers of sizes[i] bytes, n_pairs pairs (conflict_pairs[2k], conflict_pairs[2k+1]) that
 * may not overlap.  Largest buffer first (ties: lowest index), each at the lowest 256-byte aligned offset where it overlaps no conflicting
 * buffer placed before it: a deterministic function of its arguments.  offsets[i] in bytes, *total = the end of the last buffer. */
int grnet_arena_assign(int n, const int64_t* sizes, int n_pairs, const int32_t* conflict_pairs, int64_t* offsets, int64_t* total);

/* model.load_state_dict(...) -- demo.py:116-122, batch_generation.py:214-218, and
 * GRNet.load_pare_dict / load_ckpt_w_prefix -- grnet.py:93-109, lib/utils/utils.py:185-196.
 * Called once per checkpoint tensor under its REFERENCE key name ("backbone.conv1.weight",
 * "head.pose_mlp.weight", ...; GRU keys "pfeat_corrector.featnet.*" or "gru.*").  host_ptr is
 * read during the call only. */
int grnet_load_tensor(grnet_t* h, const char* state_dict_key, const void* host_ptr, const int64_t* shape, int ndim,
                      int dtype);

/* SMPL(...) buffers -- lib/models/smpl.py:97-106,144 (smplx.SMPL tables + J_regressor_extra).
 * v_template (6890,3), shapedirs (6890,3,10), posedirs (207,20670), J_regressor (24,6890),
 * lbs_weights (6890,24), parents (24), J_regressor_extra (9,6890); host pointers.  Of J_regressor_extra the non-zero entries of every row are
 * kept on the device (row 5, 'Thorax (MPII)', for the 29 joints of every forward; all nine for grnet_smooth_pose's 49). */
int grnet_load_smpl(grnet_t* h, const float* v_template, const float* shapedirs, const float* posedirs,
                    const float* J_regressor, const float* lbs_weights, const int32_t* parents,
                    const float* J_regressor_extra);

/* model.eval() + first use: folds every BatchNorm2d (eval, eps 1e-5) into its convolution in
 * fp64, repacks weights to the kernel layout and uploads them.  Fails with GRNET_ENOENT naming
 * the first missing tensor. */
int grnet_finalize_weights(grnet_t* h);

/* Caller-allocated device buffers for one call of n frames; any pointer may be NULL (that output
 * is then computed into an internal buffer and not returned).  Shapes follow VPRegressor.forward,
 * lib/models/pare.py:78-84, flattened over (B,T) -> n. */
typedef struct grnet_outputs {
    float* theta;             /* (n,85)  [cam(3), axis-angle pose(72), betas(10)]   pare.py:79 */
    float* verts;             /* (n,6890,3)                                         pare.py:80 */
    float* kp_2d;             /* (n,29,2)                                           pare.py:81 */
    float* kp_3d;             /* (n,29,3)                                           pare.py:82 */
    float* rotmat;            /* (n,24,3,3)                                         pare.py:83 */
    float* point_local_feat;  /* (n,128,24)  GRU input, grnet.py:148,163             */
    float* cam_shape_feats;   /* (n,64,24)                                          */
    float* pred_rot6d;        /* (n,24,6)   pare.py:299 */
    float* features;          /* (n,480,56,56) backbone output, hrnet.py:524 (debug / parity) */
    float* part_attn;         /* (n,25,56,56) heat-maps incl. background channel 0, pare.py:312 */
    float* smpl_feats;        /* (n,128,56,56) pare.py:323 */
} grnet_outputs_t;

/* model(batch)[-1] -- GRNet.forward, lib/models/grnet.py:129-175 (use_gait_feat=False path),
 * callers demo.py:164 and batch_generation.py:315.  frames_dev: (n,3,224,224) NCHW fp32 already
 * normalised; 1 <= n_frames <= max_frames. */
int grnet_forward(grnet_t* h, const float* frames_dev, int n_frames, const grnet_outputs_t* out, void* stream);

/* BidirectionalModel.forward -- lib/models/layers/gait_feat_encoder.py:79-104 (use_pareFeat=True,
 * eval).  x (b,T,3072) laid out c*24+j, cparams (b,T,3) -> y (b,3), phase (b,T,4), xc (b,T,3072);
 * device pointers; xc may be NULL. */
int grnet_gru_forward(grnet_t* h, const float* x_dev, const float* cparams_dev, int b, int T, float* y_dev,
                      float* phase_dev, float* xc_dev, void* stream);

/* TSAttnBlock.forward (use_jwff=True, eval) -- lib/models/layers/attention_utils.py:261-270: MultiAttention :164-217
 * (temporal attention over the n frames of a clip + spatial attention over the 25 tokens of a frame, softmax-gated),
 * JointWiseFeedForward :123-130 and the reference's own LayerNormalization :17-27, in the one-layer configuration of
 * feature_correction.py:92-101 (3072 -> 1000 -> 3072, 4 heads, 24 joints + 1 gait token).  Weights are loaded under
 * their reference keys with prefix "tsattn." or "pfeat_corrector.featTencoder.0.".  x (b,n,128,24), xs (b,n,128,25)
 * -> y (b,n,3072); device pointers. */
int grnet_tsattn_forward(grnet_t* h, const float* x_dev, const float* xs_dev, int b, int n, float* y_dev, void* stream);

/* What grnet_tsattn_forward / grnet_gait_correct do with a clip of n frames on this handle's device, computed by the functions the
 * launcher itself calls (the blocked kernel's threshold, the key-part count from the device's CU count): plan[0] temporal-attention
 * kernel (0: one workgroup per query, 1: blocked, 128 queries per workgroup), plan[1] key parts per (query tile, head) (1: the kernel
 * normalises and stores itself, no combine launch), plan[2] key blocks of 32 keys (0 for the per-query kernel), plan[3] dynamic LDS
 * bytes of the attention launch.  GRNET_EINVAL beyond the per-clip limit. */
int grnet_tsattn_plan(grnet_t* h, int n, int32_t* plan);

/* Taps of the temporal branch (tests / diagnosis).  Arms the NEXT grnet_gru_forward, grnet_tsattn_forward or grnet_gait_correct on
 * this handle (and this host thread): behind every launch of that call, a device-to-device copy of the launch's output into buf_dev is
 * enqueued on the call's stream -- the temporal scratch itself cannot be read after the call (x_t is gated in place, the key-part
 * partials share memory with y_t | y_s | x1, the GRU's gi becomes the heads' hidden buffer).  The launches, their order, their buffers
 * and their aliasing are the production ones, so the call's outputs are bit-identical armed and unarmed; unarmed, nothing extra is
 * enqueued.  A buffer smaller than what the armed call copies is refused by that call, before anything is enqueued, with the size
 * needed in grnet_last_error; the call disarms the taps either way.  buf_dev NULL or floats 0: disarm. */
int grnet_temporal_taps(grnet_t* h, float* buf_dev, size_t floats);

/* The layout of what the last armed call copied, one text line per entry: "tap <name> <offset in floats> <dims...>" in launch order
 * (names gru.*, ts.*, fc.*: the GRU, the attention block, the corrector around them; ts.part_o / ts.part_ml are the per-part
 * (O, m, l) of a clip whose keys were split), and "gemm <M> <N> <K> <slices>" for every launch of the fp32 GEMM (slices > 1: split-K).
 * buf NULL: returns the bytes needed; else the length written, or GRNET_EINVAL if buf_size is too small. */
int grnet_temporal_tap_layout(grnet_t* h, char* buf, int buf_size);

#define GRNET_OPT_USE_GRAPH 1     /* 1: capture each distinct (n, pointers) forward into a hipGraph and replay it */
#define GRNET_OPT_CONV_TILE 2     /* 0 = cost model; 7 / 14 = whole-K tiles; 1071/1072/1041/1042/1171/1141 = split-K (psw,csw[,8 waves]) (tests / tuning); any forced
                                   * tile also switches the Winograd layers back to the direct kernels */
#define GRNET_OPT_MULTI_LANE 3    /* 1 (default): independent HR-module branches run on parallel streams / graph branches */
#define GRNET_OPT_WINOGRAD 7      /* 1 (default): the 3x3 stride-1 layers on 56x56 / 28x28 maps (layer1, HR branches 0 and 1, transition1, upsample heads, PARE
                                   * head; csrc/conv_wino4.hip) and on 14x14 / 7x7 maps (HR branches 2 and 3, the 256 -> 256 upsample-head layer;
                                   * csrc/conv_wino4s.hip) run as Winograd F(4x4,3x3) on the fp32 matrix cores (4x fewer multiplies, fp32 throughout, sums
                                   * re-associated: ~1e-5 of the output scale from the direct kernel per layer, <= 3.5e-5 on the path's outputs); 0: every
                                   * convolution is the direct implicit GEMM.  grnet_op_conv2d tile hints 2001 / 2020 (+ K split) run the two kernels on
                                   * one convolution.  (Options 4, 5, 6 -- grouped launches, the persistent dataflow launch and its fence -- were removed
                                   * in round 3 after losing every measurement; their sources are in the history: commit 8d3a931.) */
#define GRNET_OPT_BF16_CHAIN 8    /* bf16 handles, a mask of the band- / frame-resident kernel groups of csrc/conv_bf16_chain.hip, conv_bf16_wide.hip, conv_bf16_s2.hip and csrc/conv_bf16.hip (default: all bits = -1;
                                   * process-wide default from the environment variable GRNET_BF16_CHAIN; 0: one launch of the generic kernel per convolution at every
                                   * call size).  Bits 0-3: the four BasicBlocks (8 convolutions, lib/models/hrnet.py:141-187) of an HR branch as ONE launch with the
                                   * frame resident in LDS, in calls of >= 64 frames -- bit 0: 64 ch @28x28, bit 1: 128 ch @14x14, bit 2: 256 ch @7x7, bit 3: 32 ch
                                   * @56x56 (one launch per BasicBlock there, 8-row bands streamed through LDS).  Bit 4: the wide 3x3 stride-1 layers (upsample
                                   * heads, PARE head, layer1's 3x3) with a band of the input resident, >= 32 frames.  Bit 5: the 3x3 stride-2 layers (fuse layers'
                                   * down paths, transitions, the stem's second convolution) with the band de-interleaved by row / column parity, >= 64 frames.
                                   * Bit 6: layer1's 64 -> 256 expansions (hrnet.py:80-100) also run the NEXT Bottleneck's 256 -> 64 reduction from the tile they
                                   * hold in LDS, >= 19 frames.  Bit 7: the 1x1 layers of layer1 and of the PARE head on the persistent stream kernel
                                   * (conv_bf16_pw_stream, bit-identical to the generic kernel), >= 42 frames.  Bit 8: each layer1 Bottleneck (hrnet.py:62-100: 1x1
                                   * reduce, 3x3, 1x1 expand + residual) and bit 9: the stem pair (hrnet.py:470-476) as ONE launch whose workgroups walk a frame row
                                   * by row with every intermediate in LDS (csrc/conv_bf16_roll.hip), >= 64 frames; they take precedence over bits 4-7 on those layers. */
#define GRNET_OPT_GRU_MODE 9      /* form of the bi-GRU recurrence (csrc/gru_kernels.hip; gait_feat_encoder.py:79-104).  3 (default): W_hh resident in registers, split over 8
                                   * workgroups per (sequence, direction), rows per wave, v_exp / v_rcp gate functions, h_t handed over inside the XCD's L2
                                   * (workgroup-scope granule stores + L1-bypassing polls) where the 8 workgroups verifiably share an XCD; 2: the same with
                                   * expf / tanhf; 1: column slices, agent-scope hand-off; 0: one workgroup per (sequence, direction) (also taken for b > 16 or
                                   * T < 8).  + 16: agent-scope granule stores whatever the placement.  The L2 hand-off relies on write-through of workgroup-scope
                                   * stores into the XCD's shared L2: if a poll ever runs into its bound the kernel sets a host-visible word, the
                                   * NEXT grnet_gru_forward / grnet_gait_correct on the handle returns GRNET_ESTATE once (the earlier call's outputs are
                                   * NaN-poisoned) and the handle moves itself to + 16, then to 0. */
#define GRNET_OPT_BF16_MIN_FRAMES 10 /* bf16 handles: smallest call (frames) from which EVERY kernel group of GRNET_OPT_BF16_CHAIN runs; 0 (default): each group's own
                                   * measured threshold (64 / 32 / 64 / 19 / 42 frames).  1 lets tests and small-batch deployments take the LDS-resident kernels
                                   * at any call size. */
int grnet_set_option(grnet_t* h, int option, int value);

/* Optional, once per distinct n_frames after grnet_finalize_weights: times every launch configuration of every
 * distinct convolution shape (and grouped vs parallel-lane scheduling of the HR modules) on this GPU and keeps the
 * fastest.  Synchronises the stream; overwrites the activation buffers.  Without it the cost model decides. */
int grnet_tune(grnet_t* h, int n_frames, void* stream, int level /* 1: per shape in isolation, 2: + greedy in-context refinement (seconds) */);
/* The tuned table of n_frames as text (returns its length) / re-apply a stored table without measuring. */
int grnet_get_tuning(grnet_t* h, int n_frames, char* buf, int buf_size);
int grnet_set_tuning(grnet_t* h, int n_frames, const char* text);

/* Introspection used by bench.py / tests. */
int grnet_num_kernel_launches(grnet_t* h);      /* launches enqueued by one grnet_forward */
/* The cross-lane hand-offs of the handle's lane schedule (csrc/lane_deps.h; what GRNET_TRACE prints as "dependencies:"): counts[GRNET_PLAN_OPS] ops of a forward,
 * WAITS_ALL / RECORDS_ALL hipStreamWaitEvent calls / recorded events per eager forward if every cross-lane read-after-write edge waited,
 * WAITS / RECORDS those the schedule keeps (an edge is dropped when its lane is already ordered behind the producer), LANES_ALL / LANES_JOINED
 * side lanes in use / side lanes the caller's stream still joins at the end.  Indices: the GRNET_PLAN_* enumerators below. */
enum { GRNET_PLAN_OPS = 0, GRNET_PLAN_WAITS_ALL, GRNET_PLAN_RECORDS_ALL, GRNET_PLAN_WAITS, GRNET_PLAN_RECORDS, GRNET_PLAN_LANES_ALL, GRNET_PLAN_LANES_JOINED, GRNET_PLAN_COUNTS };
int grnet_plan_counts(grnet_t* h, int64_t* counts /* GRNET_PLAN_COUNTS */);
int grnet_num_conv_launches(grnet_t* h);        /* convolution launches of one grnet_forward (incl. the grouped fuse-term launch of each HR module) */
double grnet_conv_flops_per_frame(grnet_t* h);  /* 2 * MACs of all convolutions on the path */
/* The same with the layers that run a Winograd F(4x4,3x3) kernel counted at the 1/4 of their multiplies it executes (x 256/196 on 14x14 and
 * x 64/49 on 7x7 maps, whose tiles are padded), under the kernel choice of the handle's latest forward (that of a 16-frame call before the
 * first one: the 7x7 layers take the Winograd kernel from 12 frames per call on).  fp32 handles with GRNET_OPT_WINOGRAD on; equal to
 * grnet_conv_flops_per_frame otherwise.  Reporting only: the roofline figure is quoted on the algorithmic count above, this one says what
 * the matrix cores were actually asked to do. */
double grnet_conv_executed_flops_per_frame(grnet_t* h);
double grnet_conv_executed_flops_per_frame_n(grnet_t* h, int n_frames);   /* the same for a call of n_frames frames, stated explicitly */
/* The pos-th convolution launch of one forward in the un-grouped launch order (the dispatch order of a
 * GRNET_OPT_MULTI_LANE=0, un-tuned run -- what tools/layer_table.py joins per-dispatch profiler rows on):
 * info[0..11] = Cin, Cout, kernel, stride, Hin, Win, Hout, Wout, fused addends, relu, lane, addend elements per
 * frame; name = state_dict key of its weight (hrnet.py / pare.py module path).  Returns 0 or GRNET_EINVAL. */
int grnet_describe_conv(grnet_t* h, int pos, int32_t* info /* 12 */, char* name, int name_size);
/* fp32 handles run the 1x1 "up" terms of an HR module's fuse layer (hrnet.py:199-210 as summed at :258-265) as ONE launch per module
 * (csrc/hr_fuse.hip); grnet_describe_conv lists it in its place with Cin = 0, Cout = the channels it writes (32 [+ 64 [+ 128]]), kernel 1,
 * the 56x56 map of output 0, "fused addends" = the module's branch count, addend elements = the floats it reads per frame, and the name
 * "<module>.fuse_layers(up)".  Multiply-accumulates per frame of the pos-th launch of that list (either kind; < 0: bad position): */
double grnet_describe_conv_macs(grnet_t* h, int pos);
/* Per-launch figures for bench.py's kernel table (positions as in grnet_describe_conv): the kernel that runs the pos-th launch in a call
 * of n_frames frames (family<shape> name) and the multiply-accumulates per frame the matrix cores execute for it; and the average
 * duration, in microseconds, of `reps` back-to-back launches of it ALONE on `stream` (HIP events around the repetitions, two warm launches
 * first; the launch reads and writes its own planned buffers, whose contents are garbage afterwards like after any forward). */
int grnet_conv_kernel_info(grnet_t* h, int pos, int n_frames, char* name, int name_size, double* executed_macs_per_frame);
int grnet_time_conv(grnet_t* h, int pos, int n_frames, int reps, void* stream, float* us_out);
/* fp32 handles: the launch form the pos-th launch (positions as in grnet_describe_conv) takes in a call of n_frames frames under the tile hint
 * in effect, as one text line "<family> key=value ...", from the launchers' own choice functions:
 *   direct split_k=<0 whole-K tiles | 1 split-K> pixel_tile= channel_tile= waves= width_variant=<edge-pointer variant's width, 0: generic> rows= hint=
 *   wino4 waves=4 nb= gx= gy= xcd= split=<1: the last round as half-size workgroups> full= rest=   |   wino4w waves=8 npw= gx= gy= xcd= split=0
 *   wino4s images_per_tile= row_tiles= partial=<1: the last row tile holds fewer images>   |   pw   |   stem   |   fuse_up
 * *tuning_index (may be NULL) receives the convolution index grnet_set_tuning's table uses for it (-1: fuse_up, which takes no hint).
 * GRNET_EINVAL (with a message) if the hint in effect is not valid for that layer or buf is too small; GRNET_ESTATE on bf16 handles. */
int grnet_conv_launch_form(grnet_t* h, int pos, int n_frames, char* buf, int size, int* tuning_index);
/* Diagnostic: ONE eager forward on the lane streams with a HIP timing event in front of and behind every op (placed after the op's
 * cross-lane waits), after two untimed warm passes; no profiler involved.  Writes one text line per op in enqueue order --
 * "index lane start_us end_us label", times relative to the first op's start -- into buf and returns the text's length (< 0: error;
 * GRNET_EINVAL if buf_size is too small).  Synchronises the stream.  tools/op_timeline.py prints concurrency and per-section sums. */
int grnet_op_timeline(grnet_t* h, const float* frames_dev, int n_frames, void* stream, char* buf, int buf_size);
/* Re-enqueue ONLY the convolution launches of the last forward, bracketed by HIP events on
 * `stream`; returns elapsed ms in *ms_out (synchronises the stream). */
int grnet_time_convs(grnet_t* h, int n_frames, void* stream, float* ms_out);

/* Single-op entry points (parity tests of each kernel against the oracle; not used by the path).
 * w_host: (Cout,Cin,ks,ks) already folded, bias_host (Cout) or NULL, add_dev: same shape as out or NULL. */
int grnet_op_conv2d(grnet_t* h, const float* in_dev, int n, int cin, int hgt, int wid, const float* w_host,
                    const float* bias_host, int cout, int ks, int stride, int relu, const float* add_dev,
                    float* out_dev, int tile_hint, void* stream);
/* bf16 handles: grnet_op_conv2d with n_add (<= 3) addends.  Addend k: (n,add_ctot[k],ho>>add_shift[k],wo>>add_shift[k]) f32 NCHW, of which
 * the launch adds channels add_coff[k] .. add_coff[k]+cout-1, nearest-upsampled by 2^add_shift[k] (the fuse layers' addend views). */
int grnet_op_conv2d_adds(grnet_t* h, const float* in_dev, int n, int cin, int hgt, int wid, const float* w_host, const float* bias_host, int cout, int ks,
                         int stride, int relu, int n_add, const float* const* adds_dev, const int* add_ctot, const int* add_coff, const int* add_shift,
                         float* out_dev, int tile_hint, void* stream);
/* (a bf16 handle runs the bf16 path's NHWC kernel between two layout conversions: c a multiple of 8) */
int grnet_op_bilinear2x(grnet_t* h, const float* in_dev, int n, int c, int hgt, int wid, float* out_dev, void* stream);
/* The attention pooling alone -- KeypointAttention.forward, lib/models/layers/keypoint_attention.py:42-48 (softmax of every joint's heat map over the
 * 3136 positions, then the matmul with the features), called twice on the same heat maps at lib/models/pare.py:331-332 -- through the forward's own
 * two launches: the pooling kernel of the handle's path (seven ranges of 448 positions, each against its own maximum) and the front of the regressor
 * tail that merges the ranges.  heat_dev (n,25,56,56) with channel 0 the background (never read into a result), feat_a_dev (n,128,56,56),
 * feat_b_dev (n,64,56,56): f32 NCHW; plf_out_dev (n,128,24) and csf_out_dev (n,64,24): f32, out[c][j] = sum_p softmax(heat[1 + j])[p] feat[c][p].
 * A bf16 handle rounds the three maps to NHWC bf16 buffers with the plan's channel strides first, as grnet_op_bilinear2x does.  Workspace and the
 * tail's other outputs are scratch of the call; any n >= 1.  Needs finalized weights (the tail runs whole); synchronises `stream`.
 * GRNET_EINVAL, with nothing written, for a NULL pointer or n < 1. */
int grnet_op_attention_pool(grnet_t* h, const float* heat_dev, const float* feat_a_dev, const float* feat_b_dev, int n, float* plf_out_dev,
                            float* csf_out_dev, void* stream);
/* bf16 handles: a chain of nconv (even, <= 8) 3x3 stride-1 convolutions c -> c on (n,c,wid,wid) maps as ONE launch with the frame resident in LDS
 * (csrc/conv_bf16_chain.hip) -- convolutions 2k, 2k+1 are conv1 / conv2 of BasicBlock k (lib/models/hrnet.py:43-59: conv-BN-ReLU, conv-BN, + block
 * input, ReLU; four of them are one branch of a HighResolutionModule, hrnet.py:141-187).  (c, wid) in {(64,28), (128,14), (256,7)}; (32,56) runs
 * one launch per BasicBlock with 19-row bands of the frame resident.
 * in_dev / out_dev: f32 NCHW device buffers (rounded to / from NHWC bf16 around the launch); w_host: nconv x (c,c,3,3) folded weights,
 * bias_host: nconv x (c).  reps > 0 and us_out != NULL: `reps` more launches are timed with HIP events (us per launch).  Synchronises. */
int grnet_op_conv_chain(grnet_t* h, const float* in_dev, int n, int c, int wid, int nconv, const float* w_host, const float* bias_host,
                        float* out_dev, int reps, float* us_out, void* stream);

/* SMPL(...) forward with rotation matrices -- lib/models/smpl.py:108-130 (smplx LBS + the 29 "spin2" joints) and, when
 * cam_dev != NULL, the projection of smpl.py:172-186.  Used by the --smooth step (lib/utils/smooth_pose.py:59-100), which
 * re-evaluates SMPL on the filtered pose.  betas (n,10), rotmat (n,24,3,3), cam (n,3) or NULL -> verts (n,6890,3),
 * kp3d (n,29,3), kp2d (n,29,2) or NULL; device pointers; n <= max_frames. */
int grnet_smpl_forward(grnet_t* h, const float* betas_dev, const float* rotmat_dev, const float* cam_dev, int n, float* verts_dev,
                       float* kp3d_dev, float* kp2d_dev, void* stream);

/* VPRegressor.forward's J_regressor override -- lib/models/pare.py:70-76 (the evaluation path: MPJPE on Human3.6M / 3DPW is computed on the
 * joints a dataset's own regressor takes from the predicted mesh): pred_joints = J_regressor (rows,6890) @ verts, then [:, H36M_TO_J14] for
 * tables of fewer than 24 rows (lib/models/smpl.py:93-94).  J_host: (rows,6890) host floats, read during the call only; any finite content
 * (dense or sparse, signed, rows of any sum).  select: n_select row indices applied after the product, or NULL for all rows; it is resolved
 * here on the host, so only the selected rows are uploaded and computed: 1 <= rows written per frame <= GRNET_JOINT_REGRESSOR_MAX_ROWS.
 * Replaces a table set earlier; J_host == NULL clears it.  Allowed before or after grnet_finalize_weights.  Allocates the table and the
 * workspace of grnet_regress_joints (sized for max_frames) and synchronises the device before it frees the table it replaces.
 * GRNET_EINVAL (with a message): rows < 1, n_select < 1, an index outside [0, rows), more rows than the limit, a non-finite entry.
 * Every failure (these, GRNET_ENOMEM, GRNET_EHIP) leaves the table set before in place: the new one is allocated and filled first. */
#define GRNET_JOINT_REGRESSOR_MAX_ROWS 64
int grnet_set_joint_regressor(grnet_t* h, const float* J_host, int rows, const int32_t* select, int n_select);
int grnet_joint_regressor_rows(grnet_t* h);      /* rows grnet_regress_joints writes per frame; 0: none set */
/* verts_dev (n,6890,3) -> joints_dev (n,Jout,3); device pointers, verts_dev 8-byte aligned; 1 <= n <= max_frames; enqueued on `stream`
 * (two launches, csrc/joint_regress.hip), no allocation, no host synchronisation.  fp32 fma chains on the fp32 matrix cores over a FIXED
 * split of the vertices: the joints of a frame are bit-identical whatever the size of the call and wherever the frame sits in it.  Whoever
 * holds `verts` calls it (after grnet_forward, grnet_head_forward, grnet_gait_correct -- on the FINAL vertices, grnet.py:171 -- or
 * grnet_smpl_forward); kp_3d of those calls stays the 29 "spin2" joints.  GRNET_ESTATE if no table is set.
 * The slice partials go through ONE workspace per handle: calls on a handle must be ordered (one stream, or events between streams), as for
 * grnet_forward's arena; a call may not overlap grnet_set_joint_regressor either (that one synchronises the device itself). */
int grnet_regress_joints(grnet_t* h, const float* verts_dev, int n, float* joints_dev, void* stream);

/* PareHead.forward + VPRegressor.forward from GIVEN pooled features -- lib/models/pare.py:271-303 (_pare_get_final_preds :338-375:
 * per-joint 128->6, Linear 1536->10/3, rot6d_to_rotmat) and :52-91 (SMPL, projection, rotmat -> axis-angle, theta packing).  This is
 * the second head pass of the use_gait_feat branch (grnet.py:165,171: head(new_point_local_feat, cam_shape_feats, ...) then the
 * regressor) and the single-op hook the tail's parity tests use.  point_local_feat (n,128,24), cam_shape_feats (n,64,24) are device
 * INPUTS; `out` as in grnet_forward (theta, verts, kp_2d, kp_3d, rotmat, pred_rot6d; map outputs are ignored). */
int grnet_head_forward(grnet_t* h, const float* point_local_feat_dev, const float* cam_shape_feats_dev, int n, const grnet_outputs_t* out,
                       void* stream);
/* The use_gait_feat branch of GRNet.forward AFTER the first head pass -- lib/models/grnet.py:154-173: camera parameters in the
 * full image from the crop camera and the box (:156-160), FeatCorrector.forward (lib/models/layers/feature_correction.py:104-157:
 * GRU gait encoder, gait-token MLPs, BatchNorm1d, one TSAttnBlock, residual), the SECOND head pass on the corrected pose features
 * (:165) and the regressor (:171).  The reference class reads names that are defined nowhere (it cannot be constructed as shipped);
 * they are bound as DESIGN.md records and tests/golden/featcorr.npz pins the result to the reference's own code run with those
 * bindings.  Inputs are the FIRST pass's results for the whole clip(s) (the temporal modules need every frame, so on several GPUs
 * this runs after the all-gather): point_local_feat (b*T,128,24), cam_shape_feats (b*T,64,24), cam = pred_cam rows [s,tx,ty] with a
 * row stride of cam_ld floats (3, or 85 to pass theta), bbox (b*T,4) [cx,cy,w,h], cimg (b*T,2) = half the image size
 * (lib/dataset/inference.py:84-85).  `out` as in grnet_head_forward for all b*T frames; `gait` may be NULL. */
typedef struct grnet_gait_outputs {
    float* pred_avg;          /* (b,3)      gait parameters, gait_feat_encoder.py:100-101 */
    float* pred_phase;        /* (b,T,4)    gait_feat_encoder.py:102                      */
    float* pred_cparam;       /* (b*T,3)    grnet.py:160,173                              */
    float* point_local_feat;  /* (b*T,128,24) corrected pose features, feature_correction.py:150 */
} grnet_gait_outputs_t;
int grnet_gait_correct(grnet_t* h, const float* point_local_feat_dev, const float* cam_shape_feats_dev, const float* cam_dev, int cam_ld,
                       const float* bbox_dev, const float* cimg_dev, int b, int T, const grnet_outputs_t* out,
                       const grnet_gait_outputs_t* gait, void* stream);

/* rot6d_to_rotmat -- lib/utils/geometry.py:395-410: (m,6) -> (m,3,3); rotation_matrix_to_angle_axis -- geometry.py:68-97 (via
 * quaternion :213-293,:159-210, NaN -> 0): (m,3,3) -> (m,3).  The device functions the tail kernel calls, exposed so the
 * reference's edge-case vectors (degenerate 6-D pairs, the four quaternion branches, near-pi rotations) reach the GPU code. */
int grnet_op_rot6d_to_rotmat(grnet_t* h, const float* rot6d_dev, int m, float* rotmat_dev, void* stream);
int grnet_op_rotmat_to_aa(grnet_t* h, const float* rotmat_dev, int m, float* aa_dev, void* stream);
/* Axis-angle -> rotation matrix as smplx.SMPL converts the poses smooth_pose.py:99 hands it (batch_rodrigues: angle = |aa + 1e-8|,
 * R = I + sin K + (1 - cos) K^2, accurate sinf / cosf): (m,3) -> (m,3,3). */
int grnet_op_aa_to_rotmat(grnet_t* h, const float* aa_dev, int m, float* rotmat_dev, void* stream);

/* ---- the --smooth step on device-resident results -- lib/utils/smooth_pose.py:28-116, lib/utils/one_euro_filter.py:5-46 ----------------------
 * OneEuroFilter as smooth_pose drives it (unit time steps, state x[0] and dx = 0): x_dev is T rows of 72 channels with a row stride of
 * ld >= 72 floats (72, or 85 with the pointer at theta + 3 to filter theta's pose columns in place) -> xhat_dev (T,72), dense.  One launch,
 * one workgroup; frames are staged through LDS in blocks of 32.  The arithmetic is the reference's float32 numpy arithmetic operation by
 * operation (one rounding each, IEEE division, no fused multiply-add): the result is BIT-IDENTICAL to the reference's, and frame t depends
 * on frames 0..t only.  T = 1 copies the frame.  GRNET_EINVAL (with a message): T < 1, ld < 72, a null pointer, a non-finite parameter. */
int grnet_op_one_euro(grnet_t* h, const float* x_dev, int ld, int T, float min_cutoff, float beta, float d_cutoff, float* xhat_dev, void* stream);

/* smooth_pose(pred_pose, pred_betas, min_cutoff, beta) for axis-angle poses: the filter above over all T frames (d_cutoff = 1), then SMPL on
 * the filtered pose with the betas of frame 0 for every frame (smooth_pose.py:97; only row 0 of betas_dev is read) and the joints in the
 * skeleton asked for: the 49 SPIN joints (smpl.py:119-121 -- what the reference's demo.py --smooth stores), the 29 'spin2' joints
 * grnet_smpl_forward returns, or the 25 kinectv2 joints convert_kps takes from those.  pose_dev: T rows with stride pose_ld >= 72;
 * pose_hat_dev (T,72), joints_dev (T,49|29|25,3) and, unless NULL, verts_dev (T,6890,3) are written.  T is NOT limited by max_frames: the
 * SMPL part runs in chunks of max_frames in stream order (Rodrigues + betas broadcast, the launches of grnet_smpl_forward, one joints
 * launch per chunk).  No host synchronisation; the only allocation is a (max_frames x 313 floats) workspace at the first call on the handle,
 * outside the activation arena.  It shares grnet_smpl_forward's workspace: calls on a handle must be ordered as for that function.
 * GRNET_EINVAL (with a message): T < 1, pose_ld < 72, a null pose / betas / pose_hat / joints pointer, an unknown joints_kind, a non-finite
 * min_cutoff or beta; GRNET_ESTATE: no SMPL tables, or before grnet_finalize_weights. */
#define GRNET_JOINTS_SPIN49   0
#define GRNET_JOINTS_SPIN2    1
#define GRNET_JOINTS_KINECTV2 2
int grnet_smooth_pose(grnet_t* h, const float* pose_dev, int pose_ld, const float* betas_dev, int T, float min_cutoff, float beta, int joints_kind,
                      float* pose_hat_dev, float* verts_dev, float* joints_dev, void* stream);

/* ---- the mesh overlay of demo.py --mesh_render -- lib/utils/renderer.py:78-126 (csrc/render_kernels.hip; the rules in full: DESIGN.md 4.5) ---------
 * What the reference asks of pyrender, on the device: one opaque triangle mesh per call of Renderer.render, a weak-perspective camera, a z-buffer,
 * and the mask composite over the frame.  GEOMETRY follows OpenGL's rules: q = M (x, -y, -z); x_ndc = sx (q.x + tx), y_ndc = sy (q.y - ty),
 * z_ndc = -q.z; window coordinates with the origin at the bottom-left, snapped to 8 sub-pixel bits; the pixel centre is the sample; faces whose
 * doubled signed area in window space is <= 0 are culled (counter-clockwise is the front); a centre exactly on an edge is covered only if the edge is
 * a top or a left edge in image space; fragments with z outside [-1, 1] are discarded; GL_LESS, the lower face index winning at equal fp32 depth;
 * image row = H - 1 - GL row.  Coverage and the winning face do not depend on execution order.  SHADING is a stated Lambert model -- ambient 0.3 and
 * the reference's three point lights at (0,-1,1), (0,1,1), (1,1,2) in q space, shade = 0.3 + sum max(0, n.l) / (pi d^2) on the interpolated
 * area-weighted vertex normal -- and is NOT pyrender's metallic-roughness shader: pixel parity with pyrender is not claimed.
 *
 * grnet_load_faces: the (n_faces,3) int32 face table of the 6890-vertex mesh (smpl.faces / SMPL_NEUTRAL.npz 'f'), host pointer; indices are
 * validated (GRNET_EINVAL names the first bad one) and the vertex -> face table of the normals is built.  Before or after
 * grnet_finalize_weights; a second call replaces the table (it synchronises the device first); a failed call leaves the earlier table in place. */
int grnet_load_faces(grnet_t* h, const int32_t* faces_host, int n_faces);
/* Draws n meshes: verts_dev (n,6890,3) and cams_dev (n,4) rows [sx, sy, tx, ty] are device pointers; colours_host (n,3), in the image's MEMORY
 * order of channels, and image_index_host (n) are host pointers; M_host: 9 floats, row-major, or NULL for the identity (the main view; the
 * reference's --sideview is the rotation by 270 degrees about y, {0,0,-1, 0,1,0, 1,0,0}).  images_dev: uint8 (F,H,W,3), in/out: byte k of a covered
 * pixel becomes floor(255 min(1, colour_k shade) + 0.5), EVERY other byte is left as it is.  Meshes aimed at the same image are drawn in call order,
 * later over earlier, each with a fresh depth buffer (the reference's loop over the persons of a frame, far to near).
 * Everything is enqueued on `stream`, no host synchronisation.  n is NOT limited by max_frames.  Workspace: ONE allocation of 128 MiB + 3.8 MiB at
 * the first call on the handle, outside the activation arena (grnet_arena_query / grnet_arena_info are unchanged): the depth images (8 bytes a
 * pixel) of one launch group share the 128 MiB, which is one 4096 x 4096 image, and 16 meshes' vertex records take the rest.  A launch group is
 * min(16, 4096 * 4096 / (H * W)) meshes of different images (7 at 1920 x 1080); the host splits the call into layers holding the k-th mesh of
 * every image and each layer into such groups, in stream order; a group is five launches and a 256-byte memset.  Depth clears and the resolve are
 * confined to each mesh's bounding box.  Calls on a handle must be ordered (one stream, or events between streams), as for grnet_forward's arena.
 * GRNET_EINVAL (with a message): n < 0, H or W outside [1, 4096], F < 1, an image_index outside [0, F), a null pointer; GRNET_ESTATE: before
 * grnet_load_faces.  n == 0 is a no-op that reads no pointer; the checks of n, H, W, F and of the face table come first, so an empty call with
 * a bad size, or on a handle without faces, is still refused. */
int grnet_render_meshes(grnet_t* h, const float* verts_dev, int n, const float* cams_dev, const float* colours_host, const int32_t* image_index_host,
                        const float* M_host, unsigned char* images_dev, int F, int H, int W, void* stream);
/* grnet_render_meshes with flags: 0 is grnet_render_meshes exactly; a bit other than those below is GRNET_EINVAL (checked first, with a message).
 * GRNET_RENDER_WIREFRAME draws demo.py --wireframe (the reference's RenderFlags.ALL_WIREFRAME, GL's polygon mode GL_LINE): nothing is filled; every
 * face that survives the same cull (doubled area > 0) is drawn as its three edges k = 0: v0->v1, 1: v1->v2, 2: v2->v0, 1-pixel lines without
 * anti-aliasing, so front faces on the far side show through.  The line rule, on the snapped integers: the edge is x-major if
 * |dx| >= |dy|, else y-major (dx = dy = 0 draws nothing); P is the major and Q the minor coordinate, the end points are ordered P_lo < P_hi and all
 * that follows is computed from (lo, hi) alone, so both draws of a shared edge are identical; major index m is covered iff
 * P_lo <= 256 m + 128 < P_hi; the minor index is n = floor((Q_lo dP + (256 m + 128 - P_lo) dQ) / (256 dP)), exact in int64, dropped outside the
 * viewport; t = (256 m + 128 - P_lo) / dP, z = z_lo + t (z_hi - z_lo), discarded outside [-1, 1]; GL_LESS as one 64-bit atomicMin on
 * (ordered(z) << 32) | (3 face + k): at equal depth the lower 3 face + k wins.  Normal and position are interpolated between the two end points
 * with the same t; shade, store, painter's order, launch groups and workspace are those of the fill. */
#define GRNET_RENDER_WIREFRAME 1u
int grnet_render_meshes_ex(grnet_t* h, const float* verts_dev, int n, const float* cams_dev, const float* colours_host, const int32_t* image_index_host,
                           const float* M_host, unsigned char* images_dev, int F, int H, int W, unsigned flags, void* stream);
/* The stages alone, on ANY small mesh: V vertices, F faces (faces_host (F,3) int32, validated against V), one camera cam_dev (4).
 * grnet_op_raster_setup: verts_dev (V,3) -> xy_dev (V,2) int32 snapped window coordinates, z_dev (V) z_ndc, normals_dev (V,3) unit vertex normals.
 * grnet_op_raster: xy_dev, z_dev as above -> winner_dev (H,W) int32 in image rows: the winning face per pixel, -1 where uncovered.
 * grnet_op_raster_lines: the same for the wireframe: 3 face + k of the winning edge per pixel, -1 where uncovered.
 * All three allocate temporaries and synchronise `stream` before they return (test hooks, like grnet_op_conv2d). */
int grnet_op_raster_setup(grnet_t* h, const float* verts_dev, int V, const int32_t* faces_host, int F, const float* cam_dev, const float* M_host,
                          int H, int W, int32_t* xy_dev, float* z_dev, float* normals_dev, void* stream);
int grnet_op_raster(grnet_t* h, const int32_t* xy_dev, const float* z_dev, int V, const int32_t* faces_host, int F, int H, int W, int32_t* winner_dev,
                    void* stream);
int grnet_op_raster_lines(grnet_t* h, const int32_t* xy_dev, const float* z_dev, int V, const int32_t* faces_host, int F, int H, int W,
                          int32_t* winner_dev, void* stream);

/* ---- the 3D skeleton view of demo.py --skeleton_view -- demo.py:303-361 without --mesh_render, lib/utils/vis.py:571-587 (csrc/skeleton_kernels.hip;
 * the rules in full: DESIGN.md 4.6) -----------------------------------------------------------------------------------------------------------
 * grnet_spin_joints: the joints of grnet_smooth_pose WITHOUT the filter and without an SMPL pass: kp29_dev (n,29,3) and verts_dev (n,6890,3) as a
 * forward (or grnet_smpl_forward) leaves them -> joints_dev (n,49|29|25,3) for GRNET_JOINTS_SPIN49 / _SPIN2 / _KINECTV2, in chunks of max_frames,
 * bit-identical to what grnet_smooth_pose writes for the same vertices and joints.  The forward emits the 29 'spin2' joints; the reference's
 * skeleton view and its body rotation (joints 27, 28, 39, 40) are defined on the 49.  No host synchronisation, no allocation.  GRNET_EINVAL: n < 0,
 * an unknown joints_kind, a null pointer; GRNET_ESTATE: no SMPL tables.  n == 0 is a no-op after those checks. */
int grnet_spin_joints(grnet_t* h, const float* kp29_dev, const float* verts_dev, int n, int joints_kind, float* joints_dev, void* stream);
/* Draws n skeletons of P points each as S wide line segments: points_dev (n,P,3) is a device pointer; segments_host (S,2) int32 point indices,
 * colours_host (S,3) uint8 in the image's MEMORY order, widths_host (S) int32 pixels in [1, 16], image_index_host (n), R_host (9 floats, row-major,
 * or NULL for the identity), proj_host (16 doubles, row-major) and window_host (4 doubles: x0, x1, y0, y1) are host pointers.  images_dev: uint8
 * (F,H,W,3), in/out.  A point p becomes p' = R p, hw = proj[3] . (p',1), (xs, ys) = proj[0,1] . (p',1) / hw; the window maps onto the centred
 * S x S square, S = min(H, W), in GL window coordinates (origin bottom-left): x_win = (W - S)/2 + S (xs - x0)/(x1 - x0), y likewise; snapped to 8
 * sub-pixel bits; depth d = proj[3][0..2] . p'.  A point is invalid if p' is not finite, hw <= 0 or a window coordinate exceeds 2^20 pixels in
 * magnitude; a segment with an invalid end draws nothing.  Lines follow OpenGL's rule for non-antialiased lines of width w on the snapped
 * integers: ends ordered and major axis chosen as for the wireframe, major index m covered iff P0 <= 256 m + 128 < P1, the column
 * n0 .. n0 + w - 1, n0 = floor((Q0 dP + (256 m + 128 - P0) dQ - (w - 1) 128 dP) / (256 dP)), inside the viewport, all at the depth interpolated at m;
 * no caps, no joins, no anti-aliasing, no shading.  ALL skeletons aimed at an image share ONE depth image: GL_LESS on
 * (ordered(d) << 32) | (r S + s), r the skeleton's rank in call order among those aimed at that image, s the segment: at equal depth the lower id
 * wins.  The three bytes of a covered pixel become the segment's colour, EVERY other byte is left as it is; image row = H - 1 - GL row.
 * Coverage and winner do not depend on execution order.  Everything is enqueued on `stream`; n is NOT limited by max_frames.  The workspace is
 * grnet_render_meshes' (ONE allocation at the first call of either); a launch group is min(16, 4096 * 4096 / (H * W)) IMAGES, and the skeletons
 * aimed at them go through in launches of up to 64, their records as kernel arguments.  No host synchronisation: the segment table is copied
 * through pinned host memory the handle owns (a ring of 4 tables of 64 KiB, allocated at the first call; a call waits only if the copy made 4 calls
 * earlier has not finished).  A group with more than 65 536 points goes through in passes over depth images cleared as a whole.  Calls on a
 * handle must be ordered, as for grnet_render_meshes.  Does not need grnet_load_faces.
 * GRNET_EINVAL (with a message): n < 0, P outside [1, 1024], S outside [0, 4096], H or W outside [1, 4096], F < 1 -- checked first, so an empty
 * call with a bad size is still refused; n == 0 is then a no-op that reads no pointer -- a null pointer, a non-finite entry of R, proj or window,
 * an empty window (x1 <= x0 or y1 <= y0), a segment index outside [0, P), a width outside [1, 16], an image_index outside [0, F), more skeletons
 * aimed at one image than r S + s holds in 31 bits.  A refused call touches no image. */
int grnet_render_segments(grnet_t* h, const float* points_dev, int n, int P, const int32_t* segments_host, int S, const unsigned char* colours_host,
                          const int32_t* widths_host, const int32_t* image_index_host, const float* R_host, const double* proj_host,
                          const double* window_host, unsigned char* images_dev, int F, int H, int W, void* stream);
/* The two stages alone, for ONE skeleton (test hooks: they allocate temporaries and synchronise `stream` before they return).
 * grnet_op_segments_setup: points_dev (P,3) -> xy_dev (P,2) int32 snapped window coordinates, INT32_MIN in both for an invalid point, and
 * depth_dev (P).  grnet_op_raster_segments: those -> winner_dev (H,W) int32 in image rows: the winning segment per pixel, -1 where uncovered. */
int grnet_op_segments_setup(grnet_t* h, const float* points_dev, int P, const float* R_host, const double* proj_host, const double* window_host, int H,
                            int W, int32_t* xy_dev, float* depth_dev, void* stream);
int grnet_op_raster_segments(grnet_t* h, const int32_t* xy_dev, const float* depth_dev, int P, const int32_t* segments_host, int S,
                             const int32_t* widths_host, int H, int W, int32_t* winner_dev, void* stream);

/* ---- one box per sequence from 2D joints -- batch_generation.py:39-93, get_bbox_from_joints2d(smooth=False) (csrc/bbox_kernels.hip) ----
 * joints_dev: float64 (sum T, K, 3) rows (x, y, score) in pixels, n_seq sequences lying back to back; frame_offsets_host: n_seq + 1 frame offsets,
 * the first 0.  Per frame, joints whose score is below `threshold` take the three components of the joint with the highest score (the first of equal
 * ones), and h = lr_y - ul_y after ul_y -= (lr_y - ul_y) 0.10.  Per sequence, the centre is the exact 1-medoid of its T K float32 points (x, y, score):
 * the point whose summed distance to all the others is smallest, the lowest index among equal sums -- the fixed point of the reference's K-medoids
 * with k = 1 -- and nw = nh = median(h) 1.1, times 1.8 if that is below 500.  bbox_dev (n_seq,4) float64 = [cx, cy, nw, nh], cx and cy float32 values
 * widened; medoid_dev (n_seq) int32 or NULL: the medoid's index into its sequence's T K points.  Distances are formed in float32 and summed in float64
 * in a fixed order with no atomics: the float64 cost of the chosen point is within (1 + 1e-6) of the minimum, and the result does not depend on
 * scheduling.  The input must be finite.  Needs no weights: works on a handle straight from grnet_create.  No host synchronisation; the only allocation
 * is a scratch buffer owned by the handle, outside the activation arena, that grows (synchronising the device) when a call is larger than any before.
 * GRNET_EINVAL (with a message, nothing is launched): K outside [1, 64], n_seq < 1, a null pointer, a non-finite threshold, frame_offsets[0] != 0, an
 * empty sequence or offsets that do not increase, a sequence of more than 4096 frames (the n x n matrix of the reference itself would be 42 GB there).
 *
 * grnet_op_medoid: the 1-medoid alone.  points_dev (n,4) float32 rows (x, y, s, pad), 16-byte aligned; point_offsets_host: n_seq + 1 point offsets,
 * the first 0, a sequence of 1 .. 262144 points; splits: column splits of the row sums, 1 .. 64, or 0 for the library's choice.  index_dev (n_seq)
 * int32 and cost_dev (n_seq) float64: the chosen row of each sequence and its summed distance.  Same refusals. */
int grnet_bbox_from_joints2d(grnet_t* h, const double* joints_dev, int K, const int32_t* frame_offsets_host, int n_seq, double threshold,
                             double* bbox_dev, int32_t* medoid_dev, void* stream);
int grnet_op_medoid(grnet_t* h, const float* points_dev, const int32_t* point_offsets_host, int n_seq, int splits, int32_t* index_dev, double* cost_dev,
                    void* stream);

/* ---- pose metrics: MPJPE, PA-MPJPE, PVE, acceleration and acceleration error (csrc/metric_kernels.hip) ---------------------------
 * The reference has no evaluation code; DESIGN.md 4.8 is the specification.  pred_dev, gt_dev: float32 (sum T, J, 3), n_seq sequences lying back
 * to back; frame_offsets_host: n_seq + 1 frame offsets, the first 0.  Every input is widened to float64 and all arithmetic is float64.
 * select_host: n_select indices into the J joints that enter the metrics (NULL with n_select 0: all J, in order); root_host: n_root indices into
 * the J joints (select does not apply to them) whose mean is subtracted from every joint of the frame, for pred and for gt each with its own mean
 * (NULL with n_root 0: nothing is subtracted).  P, G (m, 3): the selected joints of a frame after that.
 *   mpjpe     mean_j |P_j - G_j|
 *   pa_mpjpe  mean_j |s R P_j + t - G_j| for the similarity that minimises sum_j |s R P_j + t - G_j|^2: mu1, mu2 the joint means, X1 = (P - mu1)^T,
 *             X2 = (G - mu2)^T, var1 = sum X1^2, K = X1 X2^T, R the proper rotation that maximises trace(R K) (one-sided Jacobi, csrc/procrustes3.h),
 *             s = trace(R K) / var1, t = mu2 - s R mu1.  var1 == 0 (all selected pred joints equal): s = 0, R = I.
 *   pve       mean_v |pred_verts_v - gt_verts_v|: pred_verts_dev, gt_verts_dev float32 (sum T, V, 3), both or neither; not aligned in any way
 *   accel     mean_j |P[f-1]_j - 2 P[f]_j + P[f+1]_j|; accel_err: the same of P - G.  Interior frames of a sequence only.
 * per_frame_dev (sum T, 5) float64 = [mpjpe, pa_mpjpe, pve, accel, accel_err], each times `unit` (1000: metres -> millimetres).  Entries undefined
 * by structure are NaN: the two accelerations at the first and last frame of a sequence, pve without vertices.  per_seq_dev (n_seq, 5) and total_dev
 * (5): the means over the structurally defined entries, NaN where there are none; the total is formed from the sequences' sums and counts.
 * transform_dev (sum T, 13) = [s, R row-major (9), t (3)] in the inputs' own units (`unit` does not enter).  Any of the four may be NULL.
 * Fixed summation orders, no atomics: a frame's row has the same bits whatever the call's size and the frame's position in it, a sequence's means
 * the same bits whether it travels alone or with others.  The input must be finite.  Needs no weights: works on a handle straight from grnet_create.
 * No host synchronisation; the only allocation is a scratch buffer owned by the handle, outside the activation arena, that grows (synchronising
 * the device) when a call is larger than any before.
 * GRNET_EINVAL (with a message, nothing is launched, the outputs stay untouched): J outside [1, 64], n_seq < 1, a null pred_dev, gt_dev or
 * frame_offsets_host, n_select or n_root outside [1, 64] with its pointer or not 0 without it, an index outside [0, J), one vertex pointer without
 * the other, V < 1 with vertices, a non-finite unit, frame_offsets[0] != 0, an empty sequence or offsets that do not increase.
 *
 * grnet_op_procrustes: the rotation alone (test hook).  K_dev (k,9) float64 row-major -> R_dev (k,9) the proper rotation maximising trace(R K),
 * sigma_dev (k,3) the singular values of K, s1 >= s2 >= s3 >= 0.  K = 0 gives R = I.  GRNET_EINVAL: k < 1, a null pointer. */
int grnet_pose_metrics(grnet_t* h, const float* pred_dev, const float* gt_dev, int J, const int32_t* frame_offsets_host, int n_seq,
                       const int32_t* select_host, int n_select, const int32_t* root_host, int n_root, const float* pred_verts_dev,
                       const float* gt_verts_dev, int V, double unit, double* per_frame_dev, double* per_seq_dev, double* total_dev, double* transform_dev,
                       void* stream);
int grnet_op_procrustes(grnet_t* h, const double* K_dev, int k, double* R_dev, double* sigma_dev, void* stream);

/* ---- camera-space trajectory: the translation fitted to 2D joints (csrc/translation_kernels.hip, csrc/translation3.h) -------------
 * estimate_translation_np -- lib/utils/geometry.py:296-337 (SPIN's weighted least squares), per frame, with per-sequence intrinsics, a status,
 * the reprojection error, a fill of the unfitted frames and a per-sequence summary, none of which the reference has.
 * joints3d_dev float32 (frames, K3, 3) and joints2d_dev float32 (frames, K2, 3) = (x, y, confidence) in pixels: n_seq sequences lying back to back;
 * frame_offsets_host: n_seq + 1 frame offsets, the first 0, the last `frames`.  pairs_host (n_pairs, 2) int32 = (3D joint, 2D joint);
 * camera_host (n_seq, 3) float64 = (f, cx, cy) of each sequence.  Every input is widened to float64 and all arithmetic is float64.
 *   fit     a pair is used where its confidence is finite and > conf_threshold, with weight w = confidence.  u = x - cx, v = y - cy, ex = u Z - f X,
 *           ey = v Z - f Y; A = [[f^2 Sw, 0, -f Swu], [0, f^2 Sw, -f Swv], [-f Swu, -f Swv, Sw(u^2 + v^2)]], b = [f Sw ex, f Sw ey, -Sw(u ex + v ey)],
 *           the sums over the used pairs in table order; A t = b by elimination with partial pivoting
 *   reproj  the weighted mean over the used pairs of |f (X + tx, Y + ty) / (Z + tz) + (cx, cy) - (x, y)|, pixels
 *   status  0 fitted; 1 fewer than min_joints used pairs; 2 a zero pivot, a non-finite result or a used joint with Z + tz <= 0 (the reference raises
 *           LinAlgError or returns garbage); 3 filled.  t and reproj are NaN for 1 and 2
 *   fill    (fill != 0) a run of unfitted frames between two fitted ones takes numpy.linspace(prev, next, gap + 2)[1:-1] bit for bit; a run before
 *           the first or after the last fitted frame holds the nearest fitted t; a sequence without a fitted frame stays as it is.  Filled frames get
 *           status 3 and keep a NaN reproj
 * per_frame_dev (frames, 6) float64 = [tx, ty, tz, reproj, n_used, status]; per_seq_dev (n_seq, 4) float64 = [frames fitted, frames filled, mean
 * reproj over the fitted frames (NaN without one), path length sum |(J_root + t)[i+1] - (J_root + t)[i]| over consecutive frames whose t are both
 * finite]; root: a 3D joint index.  Fixed summation orders, no atomics: a frame's fit has the same bits whatever the call, a sequence's rows and
 * summary the same bits whether it travels alone or with others.  Non-finite coordinates need no check: they end in status 2.  Needs no weights:
 * works on a handle straight from grnet_create.  No host synchronisation and no allocation: everything is enqueued on `stream`.
 * GRNET_EINVAL (with a message, nothing is launched, the outputs stay untouched): a null pointer, K3 or K2 < 1, n_pairs outside [1, 64], a pair index
 * outside K3 or K2, n_seq or frames < 1, frame_offsets[0] != 0, an empty sequence or offsets that do not ascend or do not end at `frames`, a
 * non-finite or non-positive f, a non-finite centre, a non-finite or negative conf_threshold, min_joints < 2, root outside [0, K3). */
int grnet_fit_translation(grnet_t* h, const float* joints3d_dev, int K3, const float* joints2d_dev, int K2, int frames, const int32_t* frame_offsets_host,
                          int n_seq, const int32_t* pairs_host, int n_pairs, const double* camera_host, double conf_threshold, int min_joints, int root,
                          int fill, double* per_frame_dev, double* per_seq_dev, void* stream);

/* ---- per-frame boxes from 2D joints: tracked, gaps filled, smoothed (csrc/track_kernels.hip, csrc/track_boxes.h) -----------------
 * lib/utils/smooth_bbox.py (kp_to_bbox_param squared=True, get_all_bbox_params, smooth_bbox_params) and the box of lib/dataset/inference.py:57-66.
 * joints_dev float64 (sum T, K, 3) rows (x, y, score) in pixels: n_seq sequences lying back to back; frame_offsets_host: n_seq + 1 frame offsets,
 * the first 0.  1 <= K <= 64, 1 <= n_seq <= 8192.  Everything is float64, one rounding per operation.
 *   frame    a joint counts where score > vis_thresh, strictly; min and max of x and of y over those joints, height = sqrt(dx^2 + dy^2); the frame
 *            has a detection where a joint counts and height >= 0.5; then centre = (min + max) / 2, scale = 150 / height.  Non-finite joints are
 *            not refused: every test is a comparison that is false for NaN, so a frame whose min, max or height is not finite has no detection
 *   fill     start = the first detected frame, end = the last + 1; a frame between them without a detection takes, per column,
 *            numpy.linspace(prev, next, gap + 2)[1:-1] of the detected frames on either side, bit for bit (the statement of grnet_fit_translation's
 *            fill); the neighbours are found in a bitmask of 64 frames a word, by word
 *   median   (kernel_size > 1; odd, <= 31) scipy.signal.medfilt over [start, end) of each column: the window padded with zeros (pad =
 *            GRNET_TRACK_PAD_ZERO, scipy's) or with the first / last value (GRNET_TRACK_PAD_EDGE); by selection, so exact
 *   gauss    (sigma > 0; <= 16) scipy.ndimage.gaussian_filter1d with its defaults: radius r = int(4 sigma + 0.5), weights exp(-0.5 x^2 / sigma^2)
 *            over their sum (made on the host once a call), mode reflect with period 2 (end - start) however short the track; the centre term
 *            first, then the pairs (x[l - i] + x[l + i]) w[i] from i = r down to 1 (scipy's own order)
 *   box      [cx, cy, 150 / scale, 150 / scale]
 * With kernel_size = 1 and sigma = 0 the call is get_all_bbox_params alone.
 * boxes_dev (sum T, 4) float64; status_dev (sum T) int32: 0 detected, 1 interpolated, 2 outside [start, end) (box all zeros, as
 * get_smooth_bbox_params pads), 3 inside, but the smoothed scale is not a positive finite number (box all zeros) -- with GRNET_TRACK_PAD_ZERO that
 * is the reference's own result near the ends of a track, where more than half of the median's window is padding and the median is 0;
 * range_dev (n_seq, 2) int32 = [start, end), [-1, 0) for a sequence without a detection, as the reference returns.
 * No window, fill or reflection crosses a sequence; fixed orders, no atomics: a sequence's rows have the same bits whether it travels alone or with
 * others.  Needs no weights: works on a handle straight from grnet_create.  Two launches behind one small copy from pinned memory, whatever n_seq
 * and T; no host synchronisation; the scratch is the box calls' (grown on demand, outside the arena).
 * GRNET_EINVAL (with a message, nothing is launched, the outputs stay untouched): K or n_seq out of range, a null pointer, frame_offsets[0] != 0,
 * offsets that do not increase, an even kernel_size or one outside [1, 31], a negative, non-finite or too large sigma, a non-finite vis_thresh,
 * an unknown pad.
 * grnet_op_median1d / grnet_op_gauss1d: one stage alone (test hooks) on x_dev float64, n_seq columns lying back to back with their n_seq + 1
 * offsets, into out_dev (not x_dev); sigma > 0. */
#define GRNET_TRACK_PAD_ZERO 0
#define GRNET_TRACK_PAD_EDGE 1
int grnet_track_boxes(grnet_t* h, const double* joints_dev, int K, const int32_t* frame_offsets_host, int n_seq, double vis_thresh, int kernel_size,
                      double sigma, int pad, double* boxes_dev, int32_t* status_dev, int32_t* range_dev, void* stream);
int grnet_op_median1d(grnet_t* h, const double* x_dev, const int32_t* offsets_host, int n_seq, int kernel_size, int pad, double* out_dev, void* stream);
int grnet_op_gauss1d(grnet_t* h, const double* x_dev, const int32_t* offsets_host, int n_seq, double sigma, double* out_dev, void* stream);

/* ---- gait events and parameters from the 3D joints (csrc/gait_kernels.hip, csrc/gait_events.h) -------------------------------------
 * The coordinate-based events of Zeni, Richards and Higginson (Gait & Posture 27, 2008) and what a gait lab reads from them.  The reference has no
 * gait code: DESIGN.md 4.11 is the specification.
 * joints3d_dev float32 (sum T, J, 3), camera frame of the SMPL stage (x right, y down, z away), metres: n_seq sequences lying back to back;
 * frame_offsets_host: n_seq + 1 frame offsets, the first 0; joints_host: 8 indices into the J joints -- pelvis, spine-shoulder, left hip, right hip,
 * left ankle, right ankle, left foot, right foot; trans_dev: null, or float64 (sum T, 3), the camera-space translation of every frame (NaN rows
 * allowed: grnet_fit_translation's per_frame[:, :3]).  Everything is float64, one rounding per operation.
 *   axes     per frame l = lhip - rhip, u = spine_shoulder - pelvis, f = (l x u) / |l x u| (where the body faces), n = l / |l|; a frame where
 *            |l x u| or |l| is not a positive finite number is invalid: its signals are NaN, and every later test is a comparison, false for NaN
 *   signals  hL, hR = (ankle - pelvis) . f; tL, tR = (foot - pelvis) . f; wd = |(lankle - rankle) . n|; products summed x, y, z
 *   smooth   (sigma > 0; <= 16) grnet_track_boxes' Gaussian over hL, hR, tL, tR inside each sequence; a NaN spreads as far as the kernel reaches
 *   events   frame t with all of [t - window, t + window] inside its sequence: a heel strike where h(t) > 0, h(t) > h(t - i) and h(t) >= h(t + i) for
 *            i = 1 .. window, and h(t) - min over the window >= min_excursion; a toe-off where t(t) < 0, t(t) < t(t - i), t(t) <= t(t + i) and
 *            max over the window - t(t) >= min_excursion
 * events_dev (sum T) int32: bit 0 heel strike left, 1 heel strike right, 2 toe-off left, 3 toe-off right.
 * per_frame_dev (sum T, 7) float64 = [hL, hR, tL, tR (as smoothed), wd, step_length, step_width]: at a heel strike of foot X step_length =
 * h_X(t) - h_other(t) and step_width = wd(t) (of the left foot where both strike), elsewhere NaN.
 * per_seq_dev (n_seq, 18) float64: [0..3] the four counts in the order of the bits; [4] steps = pairs of consecutive heel strikes in time order
 * (a frame with both: left first) that are of opposite feet; [5, 6] step time mean and SD in seconds, (t2 - t1) / fps; [7] cadence = 60 / [5];
 * [8, 9, 10] stride time mean, SD and 100 SD / mean over consecutive heel strikes of the same foot, the left foot's strides first; [11, 12] step
 * length mean and SD at the second strike of each step, h_X - h_other of the striking foot X; [13, 14] step width mean and SD at the same frames;
 * [15] stance share in per cent: the mean, over the strides of a foot whose first toe-off after the opening strike lies before the closing strike, of
 * 100 (t_TO - t_HS) / (t_HS' - t_HS); [16] speed = [11] * [7] / 60; [17] speed along the trajectory = |P(t_b) - P(t_a)| / ((t_b - t_a) / fps) with
 * P = pelvis + trans and t_a, t_b the first and last heel-strike frames whose trans is finite.  Means are S / n with the sums in time order,
 * standard deviations two-pass with ddof = 0.  A column is NaN where its count is 0, [17] also where trans_dev is null or t_a = t_b.
 * No window, filter or search crosses a sequence; fixed orders, no atomics: a sequence's rows have the same bits whether it travels alone or with
 * others.  Needs no weights.  At most three launches (two with sigma = 0) behind one small copy from pinned memory, whatever n_seq and T; no host
 * synchronisation; the scratch is the box calls' (grown on demand, outside the arena).
 * GRNET_EINVAL (with a message, nothing is launched, the outputs stay untouched): a null required pointer, J < 1, a table index outside [0, J),
 * n_seq outside [1, 8192] (the upper end is grnet_track_boxes': the offsets travel through the same slot of the pinned ring), frame_offsets[0] != 0,
 * offsets that do not increase, fps not positive and finite, a negative, non-finite or too large
 * sigma, window outside [1, 32], a negative or non-finite min_excursion.
 * grnet_op_gait_events: the events rule alone (test hook) on signals_dev float64 (sum T, 4) = [hL, hR, tL, tR] into events_dev. */
int grnet_gait_parameters(grnet_t* h, const float* joints3d_dev, int J, const int32_t* frame_offsets_host, int n_seq, const int32_t* joints_host,
                          const double* trans_dev, double fps, double sigma, int window, double min_excursion, double* per_frame_dev, int32_t* events_dev,
                          double* per_seq_dev, void* stream);
int grnet_op_gait_events(grnet_t* h, const double* signals_dev, const int32_t* frame_offsets_host, int n_seq, int window, double min_excursion,
                         int32_t* events_dev, void* stream);

/* ---- joint-angle kinematics per gait cycle (csrc/gait_kinematics_kernels.hip, csrc/gait_angles.h) --------------------------------
 * Hip, knee, ankle, shoulder and elbow angles and the trunk's inclination over time, cut at the heel strikes grnet_gait_parameters found, put on
 * 0 .. 100 % of the gait cycle and averaged over the strides.  The reference has no such code: DESIGN.md 4.12 is the specification.
 * joints3d_dev float32 (sum T, J, 3), frame_offsets_host as for grnet_gait_parameters; events_dev int32 (sum T): its events (bits 0 and 1, the heel
 * strikes, are read); joints_host: 16 indices into the J joints -- pelvis, spine-shoulder, then left and right hip, knee, ankle, foot, shoulder,
 * elbow, wrist.  Everything is float64, one rounding per operation; the arctangent is made of + - * / and sqrt alone (csrc/gait_angles.h), so the
 * numpy statement and the kernels agree in every bit.
 *   axes     l, u, f, n as grnet_gait_parameters makes them, and w = f x n, the body's up; an invalid frame has NaN in the channels that use the axes
 *            (0 .. 3, 8, 9, 12) and numbers in the others
 *   channels in degrees: 0, 1 hip flexion left, right atan2(d . f, -(d . w)) with d = knee - hip; 2, 3 hip abduction atan2(+-(d . n), -(d . w));
 *            4, 5 knee flexion atan2(|d x s|, d . s) with s = ankle - knee; 6, 7 ankle dorsiflexion atan2(|s x g|, s . g) - 90 with g = foot - ankle;
 *            8, 9 shoulder flexion atan2(a . f, -(a . w)) with a = elbow - shoulder; 10, 11 elbow flexion atan2(|a x b|, a . b) with
 *            b = wrist - elbow; 12 trunk inclination atan2(|u x e|, u . e) from e = (0, -1, 0), the vertical of a LEVEL camera
 *   smooth   (sigma > 0; <= 16) grnet_track_boxes' Gaussian over each of the 13 columns inside each sequence
 *   strides  pairs of consecutive heel strikes t0 < t1 of the left foot (even channels and 12) or the right (odd ones); used for a channel where
 *            min_stride <= t1 - t0 <= max_stride and the channel is finite on all of [t0, t1]
 *   cycle    point p = 0 .. 100 of a stride of L frames: q = p L div 100, r = p L mod 100, x[t0 + q] + (x[t0 + q + 1] - x[t0 + q]) (r / 100.0)
 * per_frame_dev (sum T, 13) float64: the channels as smoothed.  curves_dev (n_seq, 13, 101, 2) float64: mean and SD of every cycle point over the
 * used strides.  per_seq_dev (n_seq, 13, 6) float64: [0] strides used; [1], [2] the mean over strides of the stride's maximum and minimum; [3], [4]
 * mean and SD of the stride's range of motion max - min; [5] the symmetry index 100 |ROM_L - ROM_R| / (0.5 (ROM_L + ROM_R)) of the pair's [3], the
 * same in both channels, NaN for channel 12, where either count is 0 or the denominator is not positive.  Means are S / n with the sums in time
 * order from +0.0, standard deviations two-pass with ddof = 0; NaN where no stride is used.
 * No filter or search crosses a sequence; fixed orders, no atomics: a sequence's outputs have the same bits whether it travels alone or with others.
 * Needs no weights.  At most three launches (two with sigma = 0) behind one small copy from pinned memory, whatever n_seq and T; no host
 * synchronisation; the scratch is the box calls'.
 * GRNET_EINVAL (with a message, nothing is launched, the outputs stay untouched): a null pointer, J < 1, a table index outside [0, J), n_seq outside
 * [1, 8192], frame_offsets[0] != 0, offsets that do not increase, a negative, non-finite or too large sigma, min_stride < 1, max_stride < min_stride,
 * max_stride > 4096.
 * grnet_op_gait_cycles: the strides, cycle curves and rows alone (test hook) on angles_dev float64 (sum T, 13) and events_dev. */
int grnet_gait_kinematics(grnet_t* h, const float* joints3d_dev, int J, const int32_t* frame_offsets_host, int n_seq, const int32_t* joints_host,
                          const int32_t* events_dev, double sigma, int min_stride, int max_stride, double* per_frame_dev, double* curves_dev,
                          double* per_seq_dev, void* stream);
int grnet_op_gait_cycles(grnet_t* h, const double* angles_dev, const int32_t* events_dev, const int32_t* frame_offsets_host, int n_seq, int min_stride,
                         int max_stride, double* curves_dev, double* per_seq_dev, void* stream);

/* ---- turns and straight-walking gait parameters (csrc/gait_turns_kernels.hip, csrc/gait_turns.h) ---------------------------------
 * Where the subject turns round, and the gait row's step and stride columns over the intervals that are wholly straight walking.  Called directly
 * after grnet_gait_parameters on the same joints and on what it returned.  The reference has no such code: DESIGN.md 4.13 is the specification.  The
 * default thresholds follow the inertial-sensor turn rule of El-Gohary et al. (Sensors 14, 2014) and are UNVALIDATED on the model's output.
 * joints3d_dev float32 (sum T, J, 3), frame_offsets_host and joints_host as for grnet_gait_parameters (the first four indices are read: pelvis,
 * spine-shoulder, left hip, right hip); events_dev int32 (sum T): its events; gait_rows_dev float64 (sum T, 7): its per_frame (columns 0, 1 and 4
 * are read).  Everything is float64, one rounding per operation; every test is a comparison, false for NaN.
 *   heading  g = (f_x, f_z) of grnet_gait_parameters' f: its part in the horizontal plane of a LEVEL camera; NaN of an invalid frame
 *   step     D(0) = +0; D(t) = atan2(g_x(t-1) g_z(t) - g_z(t-1) g_x(t), g_x(t-1) g_x(t) + g_z(t-1) g_z(t)) in degrees (csrc/gait_angles.h's
 *            arctangent), positive towards the subject's left; NaN where either frame is invalid or a horizontal part vanishes
 *   rate     w = D fps, then (sigma > 0; <= 16) grnet_track_boxes' Gaussian inside each sequence; a NaN spreads as far as the kernel reaches
 *   runs     maximal runs of w > edge_rate (left) and of w < -edge_rate (right); a run is a TURN where max |w| >= peak_rate, |sum D| over it (raw
 *            steps in time order from +0.0) >= min_angle and min_frames <= its length <= max_frames
 * per_frame_dev (sum T, 2) float64 = [D, w as smoothed].  phase_dev (sum T) int32: 1 a frame of a left turn, 2 of a right turn, 3 w is NaN, 0 straight
 * (a run that is no turn included).  turns_dev (n_seq, max_turns, 7) float64, in time order: [first frame, last frame (inclusive, counted inside the
 * sequence), +1 left / -1 right, sum D, (last - first + 1) / fps, max |w|, heel strikes of either foot inside the turn (a frame where both strike
 * counts two)]; rows past the count are NaN, turns past max_turns are counted but not stored.
 * per_seq_dev (n_seq, 24) float64: [0, 1, 2] turns, left, right; [3] turn frames; [4] unknown frames; [5] straight bouts (maximal runs of phase 0);
 * [6] straight frames; [7 .. 10] the means over ALL turns of duration, |angle|, peak and steps in turn (NaN without a turn); [11 .. 23] the gait
 * row's columns 4 .. 16 in that order over the intervals that are wholly straight: a step (t1, t2), a stride (t0, t1) and the stance share's stride
 * count where no frame of the closed interval has phase != 0; consecutive still means consecutive among ALL strikes.  With no frame of phase != 0,
 * [11 .. 23] equal grnet_gait_parameters' [4 .. 16] in every bit.
 * No filter or search crosses a sequence; fixed orders, no atomics: a sequence's outputs have the same bits whether it travels alone or with others.
 * Needs no weights.  Two launches behind one small copy from pinned memory, whatever n_seq and T; no host synchronisation; the scratch is the box
 * calls'.
 * GRNET_EINVAL (with a message, nothing is launched, the outputs stay untouched): a null pointer, J < 1, a table index outside [0, J) (all 8 are
 * checked), n_seq outside [1, 8192], frame_offsets[0] != 0, offsets that do not increase, fps not positive and finite, a negative, non-finite or too
 * large sigma, a negative or non-finite edge_rate, peak_rate < edge_rate (or not finite), a negative or non-finite min_angle, min_frames < 1,
 * max_frames < min_frames, max_turns outside [1, 64].
 * grnet_op_gait_turn_runs: runs, phases, the turn table and the row alone (test hook) on rates_dev float64 (sum T, 2) = [D, w]. */
int grnet_gait_turns(grnet_t* h, const float* joints3d_dev, int J, const int32_t* frame_offsets_host, int n_seq, const int32_t* joints_host,
                     const int32_t* events_dev, const double* gait_rows_dev, double fps, double sigma, double edge_rate, double peak_rate, double min_angle,
                     int min_frames, int max_frames, int max_turns, double* per_frame_dev, int32_t* phase_dev, double* turns_dev, double* per_seq_dev,
                     void* stream);
int grnet_op_gait_turn_runs(grnet_t* h, const double* rates_dev, const int32_t* events_dev, const double* gait_rows_dev, const int32_t* frame_offsets_host,
                            int n_seq, double fps, double edge_rate, double peak_rate, double min_angle, int min_frames, int max_frames, int max_turns,
                            int32_t* phase_dev, double* turns_dev, double* per_seq_dev, void* stream);

/* ---- foot contact phases and double support (csrc/gait_contacts_kernels.hip, csrc/gait_contacts.h) ---------------------------------
 * When both feet are on the ground, and from that double-support, single-support, swing and stance time.  Called directly after
 * grnet_gait_parameters on the same joints and on its events.  The reference has no such code: DESIGN.md 4.14 is the specification.  The joints are
 * root-relative, so no foot's speed in the world is known; the vector from one ankle to the other does not depend on the root and stands still
 * while both feet do.  The thresholds are UNVALIDATED on the model's output, and smoothing SHORTENS the runs (DESIGN.md 4.14 has the figures), which
 * is why sigma defaults to 0 in the Python layers.
 * joints3d_dev float32 (sum T, J, 3), frame_offsets_host and joints_host as for grnet_gait_parameters (all 8 indices are checked; entries 4 and 5,
 * the ankles, are read); events_dev int32 (sum T): its events, of which bits 0 and 1, the heel strikes, are read.  Everything is float64, one
 * rounding per operation; every test is a comparison, false for NaN.  An INTERVAL k of a sequence lies between its frames k and k + 1, 0 <= k <= T-2.
 *   vector    d(t) = left ankle - right ankle; then (sigma > 0; <= 16) grnet_track_boxes' Gaussian over each of its three columns inside the
 *             sequence; a NaN spreads as far as the kernel reaches
 *   speed     s(k) = sqrt((dx^2 + dy^2) + dz^2) fps of d(k+1) - d(k), in metres a second, sitting at time k + 1/2; row T-1 of a sequence is NaN
 *   threshold thr = speed where speed > 0, else fraction * (S / n): n the number of finite s of the sequence, S their sum in a FIXED SHAPE --
 *             blocks of 64 consecutive intervals aligned to the sequence, inside a block a balanced tree over adjacent pairs (0+1, 2+3, ..., then
 *             pairs of those), a non-finite or missing entry +0.0, the block sums added in time order from +0.0; n = 0: NaN, and no run
 *   runs      an interval is static where s(k) < thr; a run is a maximal stretch [a, b] of static intervals; it is CLOSED where a >= 1, b <= T-3 and
 *             s(a-1) and s(b+1) are finite, and then t_start = (a - 0.5) + (s(a-1) - thr) / (s(a-1) - s(a)) and
 *             t_end = (b + 0.5) + (thr - s(b)) / (s(b+1) - s(b)), in frames
 *   lead      a closed run of at most max_frames intervals is a double support LED by foot X where some frame of [a - reach, b + 1 + reach], cut to
 *             the sequence, holds a heel strike of X and none holds one of the other foot; the earliest such strike is recorded.  Every other run
 *             is unattributed: open, too long (standing), struck by both feet or by neither.
 * per_frame_dev (sum T, 4) float64 = [s, d_x, d_y, d_z as smoothed].  phase_dev (sum T) int32, of the interval that begins at the frame: 0 moving, 1
 * static and left-led, 2 static and right-led, 3 static and unattributed, 4 s is NaN (the last row of every sequence).  runs_dev (n_seq, max_runs, 6)
 * float64, ALL static runs in time order: [t_start, t_end, +1 left / -1 right / 0 unattributed, heel-strike frame, (t_end - t_start) / fps, min s over
 * the run]; of an open run columns 0, 1 and 4 are NaN, of an unattributed one column 3; rows past the count are NaN, runs past max_runs are counted
 * and used in the row but not stored.
 * per_seq_dev (n_seq, 20) float64: [0] thr; [1] S / n, about twice the walking speed; [2] static runs; [3, 4] left-led and right-led double
 * supports; [5] unattributed runs; [6, 7] double-support time in seconds, mean and SD over the attributed runs in time order; [8, 9] its mean
 * left-led and right-led; [10] 100 |L - R| / (0.5 (L + R)); then over the STRIDES -- three consecutive static runs R0, R', R1 led by X, the other
 * foot, X (an unattributed run between breaks the chain), the left foot's first -- [11] their number; [12, 13] stride time (start R1 - start R0) mean
 * and SD; [14, 15, 16] the means of stance (end R' - start R0), swing (start R1 - end R') and single support (start R' - end R0), all in seconds;
 * [17] the mean of 100 stance / stride; [18] the mean of 100 (|R0| + |R'|) / stride; [19] 100 [13] / [12].  Means are sums in the stated order over
 * the count, SDs two-pass with ddof = 0; a column is NaN where its count is 0.
 * No filter or search crosses a sequence; fixed orders, no atomics: a sequence's outputs have the same bits whether it travels alone or with others.
 * Needs no weights.  At most three launches (two with sigma = 0) behind one small copy from pinned memory, whatever n_seq and T; no host
 * synchronisation; the scratch is the box calls'.
 * GRNET_EINVAL (with a message, nothing is launched, the outputs stay untouched): a null pointer, J < 1, a table index outside [0, J) (all 8 are
 * checked), n_seq outside [1, 8192], frame_offsets[0] != 0, offsets that do not increase, fps not positive and finite, a negative, non-finite or too
 * large sigma, a negative or non-finite fraction or speed, fraction and speed both zero, reach outside [0, 8], max_frames < 1, max_runs outside
 * [1, 512].
 * grnet_op_gait_contact_runs: the threshold, runs, phases, the run table and the row alone (test hook) on speeds_dev float64 (sum T), whose last
 * entry of every sequence is not read. */
int grnet_gait_contacts(grnet_t* h, const float* joints3d_dev, int J, const int32_t* frame_offsets_host, int n_seq, const int32_t* joints_host,
                        const int32_t* events_dev, double fps, double sigma, double fraction, double speed, int reach, int max_frames, int max_runs,
                        double* per_frame_dev, int32_t* phase_dev, double* runs_dev, double* per_seq_dev, void* stream);
int grnet_op_gait_contact_runs(grnet_t* h, const double* speeds_dev, const int32_t* events_dev, const int32_t* frame_offsets_host, int n_seq, double fps,
                               double fraction, double speed, int reach, int max_frames, int max_runs, int32_t* phase_dev, double* runs_dev,
                               double* per_seq_dev, void* stream);

/* Gait regularity and symmetry WITHOUT EVENTS, from the autocorrelation of four body signals (Moe-Nilssen and Helbostad 2004, who measure trunk
 * accelerations with a sensor; these signals are joint positions of a pose model and the defaults are unvalidated on its output): step and stride
 * time as the first two dominant lags, step and stride regularity as the coefficients there, their ratio as symmetry, and a cadence that is
 * independent of the events of grnet_gait_parameters (which is the specification).  joints3d_dev (sum T, J, 3) float32, the n_seq
 * sequences back to back, frame_offsets_host (n_seq + 1) and joints_host (8) as grnet_gait_parameters takes them (the two foot entries are checked
 * but not read); trans_dev (sum T, 3) float64 or NULL; exclude_dev (sum T) int32 or NULL: a frame whose entry is not 0 does not count (the phase of
 * grnet_gait_turns: only straight walking counts).  Float64, one rounding per operation:
 *   signals  per frame, with the axes l, u, f, n of grnet_gait_parameters and u^ = u / |u|, a dot product ((x + y) + z):
 *            [0] sep = (lankle - rankle) . f; [1] lift = (lankle - rankle) . u^; [2] sway = u^ . n; [3] bob = -(pelvis_y + trans_y).  0 .. 2 are NaN in
 *            a frame without valid axes, 3 without trans or where the trans row is not finite.  0 .. 2 are ODD (a step is half a stride with the sign
 *            turned), 3 is EVEN (it repeats every step).  sigma > 0 (<= 16): scipy's Gaussian over each channel inside its sequence; a NaN spreads.
 *   validity a frame counts for a channel where its signal is finite and its exclude entry is 0; run(t) = the frames before t that do not count; a
 *            pair (t, t + m) counts where both frames count and run(t) = run(t + m): no frame between them fails.
 *   rho      n = the frames that count, mu = S / n with S their values added in time order from +0.0, d = x - mu; for m = 0 .. max_lag: N(m) = the
 *            counting pairs, A(m) = (the sum of d(t) d(t + m) over them in time order from +0.0) / N(m), rho(m) = A(m) / A(0) -- NaN where
 *            N(m) < min_pairs, N(0) < min_pairs or A(0) is not positive.  The unbiased estimator: it can pass 1 and is never clipped.
 *   peaks    m is a local maximum where rho(m-1), rho(m), rho(m+1) are defined (1 <= m <= max_lag - 1), rho(m) > rho(m-1) and rho(m) >= rho(m+1); a
 *            local minimum is one of -rho.  FIRST PEAK: the least m in [min_lag, max_lag - 1] that is a local maximum with rho(m) >= min_peak.
 *            Odd channel: the first peak is the stride lag d2; the step lag d1 is the local minimum of least rho in [d2 - (3 d2)/4, d2 - d2/4]
 *            (integer divisions; of a tie the earliest); step regularity -rho(d1).  Even channel: the first peak is d1; d2 is the local maximum of
 *            largest rho in [2 d1 - d1/2, 2 d1 + d1/2] cut to [1, max_lag - 1]; step regularity rho(d1).  A lag not found is -1.
 *   refined  lag m + 0.5 (a - c) / ((a - 2 b) + c) with a, b, c = rho(m-1), rho(m), rho(m+1); m where that denominator is 0.
 * per_frame_dev (sum T, 4) float64: the signals as smoothed.  acf_dev (n_seq, 4, max_lag + 1) float64.  per_seq_dev (n_seq, 4, 10) float64: [0] n;
 * [1] A(0); [2] d1; [3] d1 refined; [4] step regularity; [5] d2; [6] d2 refined; [7] stride regularity rho(d2); [8] symmetry [4] / [7] (NaN where [7] <=
 * 0); [9] cadence 120 fps / [6], steps a minute.  Where rho(0) is not defined everything but [0] is NaN; what hangs on a lag not found is NaN.
 * A workgroup per (sequence, channel), a lane per lag; fixed orders, no atomics: a sequence's outputs have the same bits alone or among others.
 * Needs no weights.  At most three launches (two with sigma = 0) behind one small copy from pinned memory; no host synchronisation; the scratch is
 * the box calls'.
 * GRNET_EINVAL (with a message, nothing is launched, the outputs stay untouched): a null required pointer, J < 1, a table index outside [0, J), n_seq
 * outside [1, 8192], frame_offsets[0] != 0, offsets that do not increase, fps not positive and finite, sigma outside [0, 16], max_lag outside [8, 255],
 * min_lag outside [2, max_lag - 2], min_peak outside (0, 1], min_pairs outside [2, 2^20].  Nothing is refused on the data.
 * grnet_op_gait_autocorr: validity, rho, peaks and the rows alone (test hook) on signals_dev float64 (sum T, 4). */
int grnet_gait_regularity(grnet_t* h, const float* joints3d_dev, int J, const int32_t* frame_offsets_host, int n_seq, const int32_t* joints_host,
                          const double* trans_dev, const int32_t* exclude_dev, double fps, double sigma, int max_lag, int min_lag, double min_peak,
                          int min_pairs, double* per_frame_dev, double* acf_dev, double* per_seq_dev, void* stream);
int grnet_op_gait_autocorr(grnet_t* h, const double* signals_dev, const int32_t* exclude_dev, const int32_t* frame_offsets_host, int n_seq, double fps,
                           int max_lag, int min_lag, double min_peak, int min_pairs, double* acf_dev, double* per_seq_dev, void* stream);

/* Harmonic ratios per stride of the same four body signals (Smidt et al. 1971, Menz et al. 2003, Bellanca et al. 2013, who measure trunk accelerations
 * with a sensor; these signals are joint positions of a pose model and the defaults are unvalidated on its output): over each stride between two
 * heel strikes of one foot, the amplitudes of the first harmonics of the detrended signal, the ratio of their even and odd sums, and its bounded form
 * (which is the specification).  joints3d_dev, frame_offsets_host, joints_host, trans_dev and exclude_dev as grnet_gait_regularity takes
 * them; events_dev (sum T) int32 is the `events` output of grnet_gait_parameters, of which bits 0 and 1 (the heel strikes) are read.  Float64, one
 * rounding per operation:
 *   signals  grnet_gait_regularity's, the same bits at the same sigma: sep, lift, sway ODD, bob EVEN.  sigma > 0 (<= 16) damps the higher harmonics.
 *   strides  per sequence the pairs t0 < t1 of consecutive heel strikes of the left foot in time order, then those of the right; L = t1 - t0.  A
 *            candidate is USED for a channel where min_stride <= L <= max_stride, the channel is finite and exclude is 0 on all of [t0, t1], and
 *            neither sum E, O below fails to be positive and finite.
 *   detrend  y(i) = (x(t0 + i) - x(t0)) - (x(t1) - x(t0)) ((double)i / (double)L), i = 0 .. L - 1.
 *   twiddle  (sin, cos)(2 pi j / L) without libm: r = 4j, q = r div L, m = r mod L, swapped where 2m > L with m' = L - m, phi = (1.5707963267948966 m') /
 *            L, z = phi phi, s = phi P(z), c = Q(z) by Horner with the doubles nearest to (-1)^k / (2k+1)!, k = 8 .. 0, and (-1)^k / (2k)!, k = 9 .. 0;
 *            then selection and negation alone by q and swap.  Within 2^-51 of the true value for every 6 <= L <= 255.
 *   DFT      H = min(n_harmonics, (L - 1) div 2), less one if odd; C_k = sum y(i) cos_j, S_k = sum y(i) sin_j, j = (k i) mod L, over i in time order from
 *            +0.0; a_k = sqrt(C_k C_k + S_k S_k) (2.0 / L).
 *   ratios   w_k = a_k g_k, g_k = 1, k or k k for derivative 0, 1, 2; E, O = the sums of w_k over the even and the odd k in rising k from +0.0, PE, PO
 *            those of w_k w_k.  Odd channel: HR = O / E, iHR = (100 PO) / (PE + PO); even channel: HR = E / O, iHR = (100 PE) / (PE + PO).
 * per_frame_dev (sum T, 4) float64.  strides_dev (n_seq, 4, max_strides, 6) float64: every candidate in order, [t0, t1 (inside the sequence), +1 left /
 * -1 right, H if used else 0, HR, iHR (NaN unless used)]; rows past the count NaN; candidates past max_strides are counted and used, not stored.
 * spectrum_dev (n_seq, 4, n_harmonics, 2) float64: mean and SD of a_k over the used strides whose H >= k, NaN where none.  per_seq_dev (n_seq, 4, 12)
 * float64: [0] candidates; [1] used; [2, 3] HR mean, SD; [4, 5] HR mean of the left, of the right strides; [6] (100 |[4] - [5]|) / (0.5 ([4] + [5]));
 * [7, 8] iHR mean, SD; [9] mean L of the used strides; [10] fps / [9]; [11] the least H used.  Means S / n in the candidates' order from +0.0, SDs
 * two-pass with ddof 0, NaN where the count is 0.
 * A workgroup per (sequence, channel), a wave per stride, a lane per (harmonic, cosine | sine); fixed orders, no atomics: a sequence's outputs have
 * the same bits alone or among others, and its length is not limited.  Needs no weights.  At most three launches (two with sigma = 0) behind one small
 * copy from pinned memory; no host synchronisation; the scratch is the box calls'.
 * GRNET_EINVAL (with a message, nothing is launched, the outputs stay untouched): a null required pointer, J < 1, a table index outside [0, J), n_seq
 * outside [1, 8192], frame_offsets[0] != 0, offsets that do not increase, fps not positive and finite, sigma outside [0, 16], n_harmonics odd or outside
 * [2, 32], derivative outside [0, 2], max_stride above 255, min_stride outside [6, max_stride], max_strides outside [1, 512].  Nothing is refused on
 * the data.
 * grnet_op_gait_stride_dft: the strides, spectra and rows alone (test hook) on signals_dev float64 (sum T, 4). */
int grnet_gait_harmonics(grnet_t* h, const float* joints3d_dev, int J, const int32_t* frame_offsets_host, int n_seq, const int32_t* joints_host,
                         const double* trans_dev, const int32_t* events_dev, const int32_t* exclude_dev, double fps, double sigma, int n_harmonics,
                         int derivative, int min_stride, int max_stride, int max_strides, double* per_frame_dev, double* strides_dev,
                         double* spectrum_dev, double* per_seq_dev, void* stream);
int grnet_op_gait_stride_dft(grnet_t* h, const double* signals_dev, const int32_t* events_dev, const int32_t* exclude_dev,
                             const int32_t* frame_offsets_host, int n_seq, double fps, int n_harmonics, int derivative, int min_stride, int max_stride,
                             int max_strides, double* strides_dev, double* spectrum_dev, double* per_seq_dev, void* stream);

/* Sample entropy of the same four body signals at several scales (Richman and Moorman 2000; the coarse-graining of Costa, Goldberger and Peng 2002;
 * Lamoth et al. 2011, who measure trunk accelerations with a sensor; these signals are joint positions of a pose model, 400 frames are at the short
 * end of what the measure tolerates and the defaults are unvalidated on its output): the COUNTS of matching template pairs per (sequence, channel,
 * scale), in 64-bit integers (which is the specification).  joints3d_dev, frame_offsets_host, joints_host, trans_dev and exclude_dev
 * as grnet_gait_regularity takes them.  Float64 with one rounding per operation in front of the counts:
 *   signals  grnet_gait_regularity's, the same bits at the same sigma.  A frame counts for a channel where its signal is finite and exclude is 0.
 *   y        the signal differenced `derivative` times, y_(k+1)(t) = y_k(t+1) - y_k(t): valid where the frames t .. t + derivative all count and the
 *            result is finite; the last `derivative` frames of a sequence are invalid.  From here on an invalid value is NaN.
 *   spread   n = the valid frames of y, mu = S / n, SD = sqrt(Q / (n - 1)) with S their sum and Q that of (y - mu)(y - mu), both in time order from
 *            +0.0; r = fraction SD.  NaN where n < 2.
 *   z_tau    for tau = 1 .. scales and j < N = T div tau: (y(j tau) + ... + y(j tau + tau - 1)) / tau, added in time order; NaN unless all are
 *            valid and the result is finite.  r is the scale-1 r at every scale.
 *   counts   template i, 0 <= i < N - m, is valid where z(i) .. z(i + m) all are.  B = the pairs i < j of valid templates with |z(i+k) - z(j+k)| <= r
 *            for every k < m; A = those of them with |z(i+m) - z(j+m)| <= r too.  No self-matches.  Where r is not > 0, B = A = 0.
 * per_frame_dev (sum T, 4) float64.  counts_dev (n_seq, 4, scales, 3) int64: [valid templates, B, A].  per_seq_dev (n_seq, 4, 4) float64: [n, mu, SD,
 * r].  THE LOGARITHM IS THE CALLER'S: SampEn(tau) = ln(B / A) where both are positive (and, as the Python layer holds it, at least 50 templates are
 * valid), the complexity index their sum over the scales.
 * A workgroup per (sequence, channel, scale), a lane per template, every pair once; integer counts, no atomics: a sequence's outputs have the same
 * bits alone or among others.  The work is QUADRATIC in a sequence's frames.  Needs no weights.  At most four launches (three with sigma = 0)
 * behind one small copy from pinned memory; no host synchronisation; the scratch is the box calls'.
 * GRNET_EINVAL (with a message, nothing is launched, the outputs stay untouched): a null required pointer, J < 1, a table index outside [0, J), n_seq
 * outside [1, 8192], frame_offsets[0] != 0, offsets that do not increase, a sequence of more than 32768 frames, sigma outside [0, 16], m outside
 * [1, 4], fraction not finite or outside (0, 10], derivative outside [0, 2], scales outside [1, 8].  Nothing is refused on the data.
 * grnet_op_gait_sampen: y, the spread and the counts alone (test hook) on signals_dev float64 (sum T, 4). */
int grnet_gait_entropy(grnet_t* h, const float* joints3d_dev, int J, const int32_t* frame_offsets_host, int n_seq, const int32_t* joints_host,
                       const double* trans_dev, const int32_t* exclude_dev, double sigma, int m, double fraction, int derivative, int scales,
                       double* per_frame_dev, int64_t* counts_dev, double* per_seq_dev, void* stream);
int grnet_op_gait_sampen(grnet_t* h, const double* signals_dev, const int32_t* exclude_dev, const int32_t* frame_offsets_host, int n_seq, int m,
                         double fraction, int derivative, int scales, int64_t* counts_dev, double* per_seq_dev, void* stream);

/* Local dynamic stability of the same four body signals: the short-term largest Lyapunov exponent of Rosenstein, Collins and De Luca (1993), which the
 * gait literature reports as local dynamic stability (Dingwell and Cusumano 2000; Lamoth et al. 2011; Bruijn et al. 2013 -- on a trunk sensor over
 * 100 and more strides; these signals are joint positions of a pose model, 400 frames at 20 fps hold some 15 strides, on noisy joints the slope
 * mostly measures the noise and the defaults are unvalidated on its output): every state's NEAREST NEIGHBOUR and, per k, the product of the squared
 * distances k frames later as a mantissa with an integer exponent (which is the specification).  joints3d_dev, frame_offsets_host,
 * joints_host, trans_dev and exclude_dev as grnet_gait_regularity takes them.  Float64 with one rounding per operation; every test is a comparison,
 * false for NaN:
 *   signals  grnet_gait_regularity's, the same bits at the same sigma.  A frame counts for a channel where its signal is finite and exclude is 0.
 *   y        grnet_gait_entropy's: the signal differenced `derivative` times (1, velocities, is this project's choice), NaN where invalid.
 *   points   span = (dim - 1) lag, M = T - span points, point i = y(i), y(i + lag), .., y(i + span), valid iff all are.  E = M - horizon: only the
 *            points i < E are references or neighbours, so that both can be followed for `horizon` frames.
 *   D2(a,b)  the sum over k = 0 .. dim - 1 of (y(a + k lag) - y(b + k lag)) squared, added in that order from the first term.  No square root.
 *   nn(i)    the eligible j with |i - j| > theiler and D2(i, j) > 0 of the smallest D2, among equal ones the smallest j; else -1.
 *   curve    for k = 0 .. horizon, over the i with nn(i) >= 0 in increasing i: d2 = D2(i + k, nn(i) + k) counts where > 0 and finite; (f, e) =
 *            frexp(d2); P <- P f (one rounding); (P, e') = frexp(P); S <- S + e + e'; n <- n + 1; from P = 1, S = 0, n = 0.
 * per_frame_dev (sum T, 4) float64.  nn_dev (sum T, 4) int32, sequence-relative.  pairs_dev (n_seq, 4, horizon + 1, 2) int64: [n, S].  mant_dev
 * (n_seq, 4, horizon + 1) float64: P.  THE LOGARITHM IS THE CALLER'S: the mean logarithm of the distance at k is (ln P + S ln 2) / (2 n) (as the
 * Python layer holds it, where n >= 50), and the exponent the least-squares slope of that over k = 0 .. 10 times the frames a second.
 * A workgroup per (sequence, channel, block of 256 reference points), the blocks sized by the call's longest sequence, a lane per reference point,
 * the candidates in LDS tiles; then a workgroup per (sequence, channel), a lane per k; no atomics, nothing added across lanes: a sequence's outputs
 * have the same bits alone or among others.  The work is QUADRATIC in a sequence's frames.  Needs no weights.  At most four launches (three with
 * sigma = 0) behind one small copy from pinned memory; no host synchronisation; the scratch is the box calls'.
 * GRNET_EINVAL (with a message, nothing is launched, the outputs stay untouched): a null required pointer, J < 1, a table index outside [0, J), n_seq
 * outside [1, 8192], frame_offsets[0] != 0, offsets that do not increase, a sequence of more than 32768 frames, sigma outside [0, 16], derivative
 * outside [0, 2], dim outside [2, 8], lag outside [1, 16], theiler outside [0, 4096], horizon outside [1, 63].  Nothing is refused on the data.
 * grnet_op_gait_divergence: y, the neighbours and the curve alone (test hook) on signals_dev float64 (sum T, 4). */
int grnet_gait_stability(grnet_t* h, const float* joints3d_dev, int J, const int32_t* frame_offsets_host, int n_seq, const int32_t* joints_host,
                         const double* trans_dev, const int32_t* exclude_dev, double sigma, int derivative, int dim, int lag, int theiler, int horizon,
                         double* per_frame_dev, int32_t* nn_dev, int64_t* pairs_dev, double* mant_dev, void* stream);
int grnet_op_gait_divergence(grnet_t* h, const double* signals_dev, const int32_t* exclude_dev, const int32_t* frame_offsets_host, int n_seq,
                             int derivative, int dim, int lag, int theiler, int horizon, int32_t* nn_dev, int64_t* pairs_dev, double* mant_dev, void* stream);

/* The Welch power spectral density of the same four body signals (Welch 1967; the band 0.5 to 3 Hz and the width of the dominant peak of Weiss et
 * al. 2011, the spectral measures of Sejdic et al. 2014 -- on a trunk accelerometer; these signals are joint positions of a pose model, at 20 fps
 * and 64-frame segments the Hann window alone makes a peak about 0.45 Hz wide at half height, and the defaults are unvalidated on its output): an
 * averaged, windowed, zero-padded periodogram and thirteen columns read off it (which is the specification).  joints3d_dev,
 * frame_offsets_host, joints_host, trans_dev and exclude_dev as grnet_gait_regularity takes them.  Float64 with one rounding per operation; sine and
 * cosine are the harmonics call's own (no library); every test is a comparison, false for NaN:
 *   signals  grnet_gait_regularity's, the same bits at the same sigma.  A frame counts for a channel where its signal is finite and exclude is 0.
 *   y        grnet_gait_entropy's: the signal differenced `derivative` times (2, accelerations, as the papers measure), NaN where invalid.
 *   segments of `segment` = L frames, `hop` apart, inside every run of valid y from the run's first frame while the whole segment fits; runs and
 *            segments in time order.  candidates = their number; used = candidates where >= min_segments, else 0 (psd NaN, the row NaN behind used).
 *   segment  mu = (sum of y in time order) / L; w_i = 0.5 - 0.5 cos(2 pi i / L); v_i = (y_i - mu) w_i, zero-padded to nfft = N; for k = 0 .. N / 2
 *            C = sum v_i cos(2 pi k i / N), S = sum v_i sin(..) in rising i from +0.0, the table indexed by (k i) mod N; W2 = sum w_i^2.
 *   P(k)     (g sum_s (C^2 + S^2)) / ((used fps) W2), g = 2 for 0 < k < N / 2, else 1: scipy.signal.welch(window='hann', detrend='constant',
 *            scaling='density', nfft=N) of every run, averaged over all segments.
 *   row      n (valid y), candidates, used, band_power (sum of P fps / N over the bins within [f_lo, f_hi]), total_power (k >= 1), peak_bin (the
 *            largest positive P of the band, the smallest k of a tie; NaN of none), peak_hz (a parabola through the three bins where the peak is
 *            one, else the bin), peak_height, peak_width_hz (between the half-height crossings nearest the peak, linear between bins; NaN where a
 *            side does not cross), dominance (the three bins round the peak inside the band over band_power), centroid_hz, edge_hz (the first bin
 *            where the running band sum reaches 0.95 of it), cadence (steps a minute: 120 peak_hz on sep, lift and sway, 60 peak_hz on bob).
 * per_frame_dev (sum T, 4) float64.  psd_dev (n_seq, 4, nfft / 2 + 1) float64.  per_seq_dev (n_seq, 4, 13) float64.  THE LOGARITHM IS THE
 * CALLER'S: the spectral entropy of the band is taken from psd on the host (as the Python layer does).
 * One wave per (sequence, channel, block of 64 bins), a lane per bin, the signal, the tables and the segments in LDS; then a wave per (sequence,
 * channel) for the row; no atomics, nothing added across lanes: a sequence's outputs have the same bits alone or among others.  Needs no weights.
 * At most four launches (three with sigma = 0) behind one small copy from pinned memory; no host synchronisation; the scratch is the box calls'.
 * GRNET_EINVAL (with a message, nothing is launched, the outputs stay untouched): a null required pointer, J < 1, a table index outside [0, J), n_seq
 * outside [1, 8192], frame_offsets[0] != 0, offsets that do not increase, a sequence of more than 32768 frames, sigma outside [0, 16], fps not
 * positive and finite, derivative outside [0, 2], segment odd or outside [8, 256], hop outside [segment / 8, segment], nfft odd or outside
 * [segment, 1024], not 0 < f_lo < f_hi <= fps / 2, min_segments outside [1, 2^20].  Nothing is refused on the data.
 * grnet_op_gait_welch: y, the densities and the rows alone (test hook) on signals_dev float64 (sum T, 4). */
int grnet_gait_spectrum(grnet_t* h, const float* joints3d_dev, int J, const int32_t* frame_offsets_host, int n_seq, const int32_t* joints_host,
                        const double* trans_dev, const int32_t* exclude_dev, double fps, double sigma, int derivative, int segment, int hop, int nfft,
                        double f_lo, double f_hi, int min_segments, double* per_frame_dev, double* psd_dev, double* per_seq_dev, void* stream);
int grnet_op_gait_welch(grnet_t* h, const double* signals_dev, const int32_t* exclude_dev, const int32_t* frame_offsets_host, int n_seq, double fps,
                        int derivative, int segment, int hop, int nfft, double f_lo, double f_hi, int min_segments, double* psd_dev, double* per_seq_dev,
                        void* stream);

/* Arm swing and inter-limb coordination (the magnitude-squared coherence by Welch's overlapped segments of Carter, Knapp and Nuttall 1973; on arms
 * and legs in gait Wagenaar and van Emmerik 2000, Plotnik et al. 2007, Mirelman et al. 2016 -- these signals are joint-position angles of a pose
 * model over some 15 strides: with K segments the coherence of two unrelated signals is about 1 / K, 0.09 at the 11 segments of 400 frames, and with
 * one segment it is identically 1; the defaults are unvalidated on the model's output and the numbers are reported, never judged): the auto and
 * cross spectra of four limb angles and the rows read off them (which is the specification).  joints3d_dev, frame_offsets_host and
 * exclude_dev as grnet_gait_spectrum takes them, joints_host the 16 indices of grnet_gait_kinematics.  Float64 with one rounding per operation; sine,
 * cosine and arctangent are the library's own (no libm); every test is a comparison, false for NaN:
 *   signals  arm_left, arm_right, leg_left, leg_right in degrees: the shoulder and the hip flexion of grnet_gait_kinematics, its per-frame
 *            columns 8, 9, 0 and 1 in every bit at the same sigma (default 0).
 *   y        each signal differenced `derivative` times (default 0: amplitudes are degrees).  A frame counts iff ALL FOUR values are finite and
 *            exclude is 0: one mask for the call, so every limb and every pair is estimated on the same segments.  n = such frames.
 *   segments grnet_gait_spectrum's rule on that one mask: `segment`, `hop`, candidates, used (0 below min_segments, which is 2 .. 2^20, default 4).
 *   bin      per channel c the segment's C_c and S_c as grnet_gait_spectrum makes them; over the segments in order from +0.0: A_c += C_c C_c + S_c
 *            S_c and, for the pairs (a, b) = (0,1), (2,3), (0,3), (1,2), (0,2), (1,3): Re += C_a C_b + S_a S_b, Im += S_a C_b - C_a S_b -- the
 *            sign of scipy.signal.csd(a, b), conj(X_a) X_b: a positive phase means b leads a.  Every sum is scaled as P(k) is, the sign passes.
 *   limbs    grnet_gait_spectrum's thirteen columns of each auto row; cadence = 120 peak_hz (a limb swings once a stride).
 *   pairs    used; peak_bin: the bin of [f_lo, f_hi] with the largest positive finite M2 = Re Re + Im Im, the smallest k of a tie (NaN of none, and
 *            every column behind it); peak_hz = (k fps) / nfft; cross_amplitude = sqrt(M2); coherence_peak = M2 / (P_aa P_bb) where the product
 *            is positive and finite, NOT clamped; phase_peak = atan2(Im, Re) in degrees; phase_deviation = |phase| for an arm with the other
 *            side's leg (pairs 2 and 3), |180 - |phase|| for the four pairs expected in antiphase; lag_seconds = phase_peak / (360 peak_hz);
 *            coherence_band: the mean of the defined coherences over the band's bins in rising k from +0.0; coherence_bins: their number.
 * THE REST IS THE CALLER'S (as the Python layer does it, pipeline.coordination_rows): amplitude = sqrt(2 band_power) per limb, arm and leg
 * asymmetry = 100 |L - R| / (0.5 (L + R)), arm_leg_ratio = (0.5 (arm_left + arm_right)) / (0.5 (leg_left + leg_right)), phase_deviation_mean over
 * the pairs where it is defined; NaN where a denominator is not positive.
 * per_frame_dev (sum T, 4) float64.  auto_dev (n_seq, 4, nfft / 2 + 1).  cross_dev (n_seq, 6, nfft / 2 + 1, 2): Re, Im.  limbs_dev (n_seq, 4, 13).
 * pairs_dev (n_seq, 6, 10).  One wave per (sequence, block of 64 bins), a lane per bin for all four channels and all six pairs, the signals, the
 * tables and the segments in LDS; then a wave per (sequence, row); no atomics, nothing added across lanes: a sequence's outputs have the same bits
 * alone or among others.  Needs no weights.  At most four launches (three with sigma = 0) behind one small copy from pinned memory; no host
 * synchronisation; the scratch is the box calls'.
 * GRNET_EINVAL (with a message, nothing is launched, the outputs stay untouched): what grnet_gait_spectrum refuses, with the 16-joint table and
 * min_segments outside [2, 2^20] (one segment is refused by the rule).  Nothing is refused on the data.
 * grnet_op_gait_cross_welch: y, the densities and the rows alone (test hook) on signals_dev float64 (sum T, 4). */
int grnet_gait_coordination(grnet_t* h, const float* joints3d_dev, int J, const int32_t* frame_offsets_host, int n_seq, const int32_t* joints_host,
                            const int32_t* exclude_dev, double fps, double sigma, int derivative, int segment, int hop, int nfft, double f_lo, double f_hi,
                            int min_segments, double* per_frame_dev, double* auto_dev, double* cross_dev, double* limbs_dev, double* pairs_dev, void* stream);
int grnet_op_gait_cross_welch(grnet_t* h, const double* signals_dev, const int32_t* exclude_dev, const int32_t* frame_offsets_host, int n_seq, double fps,
                              int derivative, int segment, int hop, int nfft, double f_lo, double f_hi, int min_segments, double* auto_dev,
                              double* cross_dev, double* limbs_dev, double* pairs_dev, void* stream);

/* Footprints on the floor, the centre of mass over them and the margin of stability at foot placement (Hof, Gagey and Halbertsma 2005; the segment
 * masses after Winter 2009 and Dempster 1955; stride length and step width on the footprints against the line of progression, as a walkway such as
 * GAITRite defines them, Webster et al. 2005) WITHOUT A CAMERA MODEL (which is the specification).  The joints are root-relative,
 * but a foot on the ground stands still in the world: at a heel strike both feet are down, so the vector from the stance ankle to the landing one
 * is a world vector, and while foot X is planted COM - ankle_X is the world path of the COM up to a constant.  THE FLOOR IS THE x-z PLANE OF A
 * LEVEL, FIXED CAMERA (x right, y down, z away); the stance ankle creeps forward at heel rise, which biases speed and margins; the segment layout
 * on these joints is this project's and UNVALIDATED; a margin of a few centimetres carries about two of noise per step (DESIGN.md 4.22 has the
 * figures).  Numbers are reported, never judged.
 * joints3d_dev float32 (sum T, J, 3), frame_offsets_host and joints_host as for grnet_gait_parameters (all 8 indices are checked; entries 4 and 5,
 * the ankles, are read); events_dev int32 (sum T): its events, of which bits 0 and 1, the heel strikes, are read.  segments_host int32 (n_seg, 2):
 * proximal and distal joint; seg_weights_host float64 (n_seg, 2): mass and the COM's fraction from the proximal joint; 1 <= n_seg <= 16.
 * Everything is float64, one rounding per operation, float32 widened first; every test is a comparison, false for NaN; sums run in the stated order
 * from +0.0.
 *   1 COM     per component c = (sum_i m_i (P_i + p_i (D_i - P_i))) / (sum_i m_i), both sums in table order; rL = c - left ankle, rR = c - right ankle
 *   2 marks   the frames with a heel-strike bit, in time order; a frame with both bits is a mark and a strike of neither foot
 *   3 step    consecutive marks (t1 of foot X, t2 of foot Y) with X != Y, window <= t2 - t1 <= max_step, tb = t2 + settle inside the sequence, rX
 *             finite on all of [t1, t2], b = rX(tb) - rY(tb) finite, and rule 4's sp positive and finite and l > 0
 *   4 margin  k_i = i - window / 2.0, i = 0 .. window; N = sum k_i rX(t2 - window + i) (x and z), D = sum k_i k_i; v = (N / D) fps;
 *             sp = sqrt(v_x^2 + v_z^2); a = (v_x / sp, v_z / sp); left = (-a_z, a_x); l = -rX_y(t2); w0 = sqrt(gravity / l);
 *             xi = (rX_x(t2) + v_x / w0, rX_z(t2) + v_z / w0); MoS_AP = (b_x - xi_x) a_x + (b_z - xi_z) a_z;
 *             MoS_ML = s_Y ((b_x - xi_x) left_x + (b_z - xi_z) left_z), s_Y = +1 where Y is the left foot, -1 where the right
 *   5 chains  a chain is a maximal run of consecutive pairs that are steps; G_0 = +0, G_{j+1} = G_j + b_j per component in time order, ONE lane
 *   6 strides of a step j >= 1 of its chain: q = G_{j+1} - G_{j-1} (x, z), L = sqrt(q_x^2 + q_z^2), counted where L > 0, p = q / L, step length
 *             b_j . p, step width |b_j . (-p_z, p_x)|
 *   7 path    W(t) = G_j + rX(t) of the step with the largest t1 <= t among those whose [t1, t2] holds t
 *   8 excursions of a step j >= 1 over the frames t1 of step j - 1 .. t2 of step j (each frame on the stance of rule 7's step): max - min of W_y,
 *             and (where L > 0) of (W_x - G_{j-1,x}) (-p_z) + (W_z - G_{j-1,z}) p_x
 * per_frame_dev (sum T, 8) float64 = [c (3), W (3; NaN outside a step), stance side +1 left / -1 right / 0 none, chain number or NaN].
 * steps_dev (n_seq, max_steps, 15) float64 in time order: [t1, t2, s_Y, chain, G_{j+1} (3), stride length, step length, step width, sp, MoS_AP,
 * MoS_ML, vertical excursion, lateral excursion]; rows past the count are NaN, steps past max_steps are counted, chained and used in the row but
 * not stored.
 * per_seq_dev (n_seq, 24) float64: [0] strikes (marks with one bit); [1] steps; [2] chains; [3] strides; then mean and SD of [4, 5] stride length,
 * [6, 7] step length, [8, 9] step width; [10] 100 |L - R| / (0.5 (L + R)) of the mean step length by landing side; [11, 12] sp; [13] ground
 * speed (sum sqrt(b_x^2 + b_z^2)) / (sum (t2 - t1) / fps) over all steps; [14, 15] MoS_AP; [16, 17] MoS_ML; [18, 19] mean MoS_ML of left and of
 * right landings; [20, 21] vertical and [22, 23] lateral excursion.  Means are sums in time order over the count of values that are not NaN, SDs
 * two-pass with ddof = 0; a column is NaN where its count is 0.
 * No filter or search crosses a sequence; fixed orders, no atomics: a sequence's outputs have the same bits whether it travels alone or with others.
 * Needs no weights.  Three launches behind one small copy from pinned memory, whatever n_seq and T; no host synchronisation; the scratch is the box
 * calls'.
 * GRNET_EINVAL (with a message, nothing is launched, the outputs stay untouched): a null pointer, J < 1, a table or segment index outside [0, J),
 * n_seq outside [1, 8192], frame_offsets[0] != 0, offsets that do not increase, n_seg outside [1, 16], a mass not positive and finite, a
 * non-finite fraction, fps or gravity not positive and finite, window outside [1, 16], settle outside [0, 4], max_step < 1, max_steps outside
 * [1, 1024].
 * grnet_op_gait_balance_steps: rules 2 to 8 alone (test hook) on rel_dev float64 (sum T, 9) = [c, rL, rR]. */
int grnet_gait_balance(grnet_t* h, const float* joints3d_dev, int J, const int32_t* frame_offsets_host, int n_seq, const int32_t* joints_host,
                       const int32_t* events_dev, const int32_t* segments_host, const double* seg_weights_host, int n_seg, double fps, double gravity,
                       int window, int settle, int max_step, int max_steps, double* per_frame_dev, double* steps_dev, double* per_seq_dev, void* stream);
int grnet_op_gait_balance_steps(grnet_t* h, const double* rel_dev, const int32_t* events_dev, const int32_t* frame_offsets_host, int n_seq, double fps,
                                double gravity, int window, int settle, int max_step, int max_steps, double* per_frame_dev, double* steps_dev,
                                double* per_seq_dev, void* stream);
/* grnet_gait_balance on a centre of mass the caller brings: com_dev float64 (sum T, 3), e.g. columns 1 to 3 of grnet_mesh_moments' rows, in place of
 * the segment table.  Rule 1 becomes [c, c - left ankle, c - right ankle] with that c; rules 2 to 8, the outputs, the launches and every other
 * refusal are grnet_gait_balance's.  A frame whose c is NaN is a frame without a centre of mass, as there. */
int grnet_gait_balance_com(grnet_t* h, const float* joints3d_dev, int J, const int32_t* frame_offsets_host, int n_seq, const int32_t* joints_host,
                           const int32_t* events_dev, const double* com_dev, double fps, double gravity, int window, int settle, int max_step, int max_steps,
                           double* per_frame_dev, double* steps_dev, double* per_seq_dev, void* stream);

/* Volume, centre of mass, central second moments and surface area of the closed mesh of every frame (which is the specification).
 * verts_dev float32 (n, 6890, 3): the vertices a forward call left on the device; the face table is grnet_load_faces'.  Float64 throughout, one
 * rounding per operation, every comparison false for NaN.  Per frame: the origin o is the vertex the table's first index names, every corner is
 * taken relative to it; a face with corners a, b, c gives d = a . (b x c), s = a + b + c and the eleven terms d, d s_k, d (a_k a_l + b_k b_l +
 * c_k c_l + s_k s_l) for xx, yy, zz, xy, xz, yz, and |(b - a) x (c - a)|; column l of 1024 adds the terms of faces l, l + 1024, ... in rising order
 * from +0.0, and the columns are reduced by the fixed tree col[l] += col[l + h], h = 512 .. 1.
 * rows_dev float64 (n, 11): [0] volume = S0 / 6 in cubic metres; [1..3] the centre of mass o + S_k / (4 S0); [4..9] the central second moments per
 * unit volume S_kl / (20 S0) - m_k m_l in square metres, xx, yy, zz, xy, xz, yz (the covariance of a UNIFORM mass distribution); [10] the area
 * S10 / 2.  Where S0 > 0 is false (a mesh turned inside out, a degenerate one, a NaN) columns 1 to 9 are NaN, volume and area are stored as they
 * come.  A non-finite vertex the table names makes its frame's row NaN by the arithmetic alone; one the table does not name changes nothing.
 * sums_dev float64 (n, 11) or NULL: S0 .. S10.
 * UNIFORM DENSITY IS AN ASSUMPTION; THE MESH IS A STATISTICAL BODY SHAPE, NOT THE SUBJECT'S; the numbers are reported, never judged.
 * One launch, a workgroup per frame; fixed orders, no atomics: a frame has the same bits alone or among others.  Needs no weights: works before
 * grnet_finalize.  No host synchronisation.
 * GRNET_EINVAL (with a message, nothing is launched, the outputs stay untouched): a null verts_dev or rows_dev, n < 1, a face table that is not a
 * closed, consistently oriented surface (the message carries the count of grnet_faces_closed).  GRNET_ESTATE: no face table loaded.
 * grnet_op_mesh_moments: the same with the form of the gather named (timing hook): 0 the corners read from global memory, 1 the frame's vertices
 * staged in LDS first.  The bits do not depend on it.
 * grnet_faces_closed: host only.  *unmatched_edges_host = how many of the table's 3 F directed edges (i, j) share their pair with another edge,
 * have no reverse edge (j, i), or join a vertex to itself; 0 for a closed, consistently oriented surface.  Counted (a sort of 3 F keys) at the first
 * call after grnet_load_faces and kept. */
int grnet_mesh_moments(grnet_t* h, const float* verts_dev, int n, double* rows_dev, double* sums_dev, void* stream);
int grnet_op_mesh_moments(grnet_t* h, const float* verts_dev, int n, double* rows_dev, double* sums_dev, int form, void* stream);
int grnet_faces_closed(grnet_t* h, int* unmatched_edges_host);

/* The samples behind the gait call's step and stride columns, one row per step and per stride (which is the specification).
 * events_dev int32 (sum T) and per_frame_dev float64 (sum T, 7) as grnet_gait_parameters returned them, frame_offsets_host as there; phase_dev int32
 * (sum T): the per-frame phase of grnet_gait_turns, or null.  With phase_dev and straight_only != 0 only the steps and strides are listed that the
 * straight columns of grnet_gait_turns count: no frame of [opening strike, closing strike] has a phase other than 0.
 *   step    consecutive heel strikes in time order (the left foot first where both strike in one frame) on different feet, pt and t with the landing
 *           foot F: [pt, t, F (0 left, 1 right), (t - pt) / fps, row_t[F] - row_t[1 - F], row_t[4]]
 *   stride  consecutive heel strikes t0, t1 of one foot: [t0, t1, foot, (t1 - t0) / fps]; the left foot's strides first, then the right foot's
 * steps_dev (n_seq, max_rows, 6), strides_dev (n_seq, max_rows, 4) float64, NaN rows past the count; counts_dev int32 (n_seq, 2): the steps and the
 * strides found -- those past max_rows are counted, not stored.  Mean, SD and CV of these columns in row order ARE columns 5, 6, 8 .. 14 of the gait
 * call's row (straight-only: of the turn call's straight columns) in every bit.
 * One launch behind one small copy from pinned memory, a workgroup per sequence, no atomics, no host synchronisation; the scratch is the box calls'.
 * GRNET_EINVAL (with a message, nothing is launched, the outputs stay untouched): a null pointer other than phase_dev, straight_only without
 * phase_dev, fps not positive and finite, max_rows outside [1, 1024], n_seq outside [1, 8192], frame_offsets[0] != 0, offsets that do not increase. */
int grnet_gait_step_tables(grnet_t* h, const int32_t* events_dev, const double* per_frame_dev, const int32_t* frame_offsets_host, int n_seq, double fps,
                           int max_rows, const int32_t* phase_dev, int straight_only, double* steps_dev, double* strides_dev, int32_t* counts_dev, void* stream);

/* Nonparametric bootstrap of the mean, the SD and the CV of columns of a per-step table (Efron 1979; with block > 1 the circular block bootstrap of
 * Politis and Romano 1992; DESIGN.md 4.23, which is the specification).  A PERCENTILE INTERVAL FROM SOME 15 STRIDES UNDER-COVERS (about 0.91 where 0.95
 * is asked), steps within a walk are serially correlated, which block addresses only partly (2 keeps a left and a right step
 * together); numbers are reported, never judged.
 * table_dev float64 (n_seq, max_rows, C): any table of this layout -- the two above, grnet_gait_balance's steps; counts_dev int32 (n_seq): the rows n
 * of each sequence, a count above max_rows is read as max_rows (below 0 as 0); cols_host int32 (n_cols): the columns to resample; quantiles_host int32
 * (n_q) in basis points.
 *   generator  uint64, wrapping: G = 0x9E3779B97F4A7C15; mix(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9, z = (z ^ z >> 27) * 0x94D049BB133111EB,
 *              z ^ z >> 31; u(seed, stream, r, j) = mix(mix(mix(seed + G (stream + 1)) + G (r + 1)) + G (j + 1)); index(u, n) = ((u >> 32) n) >> 32,
 *              whose bias is below n / 2^32: stated, not corrected
 *   resample   by rows -- all columns of a replicate share the indices.  Replicate 0 is the sample, idx(p) = p; replicate r = 1 .. B has idx(p) =
 *              (index(u(seed, stream, r, p / block), n) + p % block) % n, p = 0 .. n - 1.  The draws do not depend on the sequence's place in the
 *              call: a sequence has the same bits alone or among others, and TWO SEQUENCES WITH EQUAL n GET EQUAL INDICES
 *   statistics per replicate and column in float64, one rounding per operation, over p in order from +0.0, skipping NaN values, m the count kept:
 *              mean = S / m, SD = sqrt(sum (x - mean)^2 / m), CV = (100 SD) / mean; all NaN where m = 0
 *   selection  per statistic the replicates 1 .. B that are not NaN, ordered by (value under <, then replicate number), f their count; a quantile q is
 *              the element of rank (q (f - 1)) / 10000 by integer division, NaN where f = 0
 * out_dev float64 (n_seq, n_cols, 3, 2 + n_q): per statistic [replicate 0, f, the quantiles]; replicates_dev float64 (n_seq, n_cols, 3, B): the
 * replicates 1 .. B, or null.
 * One launch whatever n_seq, a workgroup per (sequence, column, statistic), lanes over replicates; no atomics, no float sum across lanes, no scratch, no host
 * synchronisation.
 * GRNET_EINVAL (with a message, nothing is launched, the outputs stay untouched): a null pointer other than replicates_dev (quantiles_host may be
 * null where n_q is 0), n_seq outside [1, 8192], max_rows outside [1, 1024], C outside [1, 16], n_cols outside [1, 8], a column outside [0, C), B
 * outside [1, 4096], block outside [1, 1024], stream_id outside [0, 65535], n_q outside [0, 5], a quantile outside [0, 10000]. */
int grnet_bootstrap_table(grnet_t* h, const double* table_dev, const int32_t* counts_dev, int n_seq, int max_rows, int C, const int32_t* cols_host, int n_cols,
                          int B, int block, uint64_t seed, int stream_id, const int32_t* quantiles_host, int n_q, double* out_dev, double* replicates_dev,
                          void* stream);

/* Movement smoothness of the same four body signals: the spectral arc length (SPARC) and the dimensionless jerk of Balasubramanian, Melendez-Calderon,
 * Roby-Brami and Burdet 2015, per segment of ongoing walking (on gait: Beck et al. 2018 -- with a sensor at 100 Hz and more; THESE SIGNALS ARE JOINT
 * POSITIONS OF A POSE MODEL AT 20 FPS, WHERE THE CUT-OFF OF 10 HZ IS THE NYQUIST FREQUENCY; A SEGMENT CUT OUT OF WALKING HAS A RECTANGULAR WINDOW,
 * WHOSE LEAKAGE ALONE GIVES A NOISELESS SINUSOID SPARC = -3.96 +- 0.30 AT 64 FRAMES; WITH 5 MM OF JOINT NOISE A GOOD PART OF THE NUMBER IS THE NOISE;
 * THE DEFAULTS ARE UNVALIDATED ON THE MODEL'S OUTPUT: DESIGN 4.24, which is the specification).  joints3d_dev, frame_offsets_host, joints_host,
 * trans_dev and exclude_dev as grnet_gait_regularity takes them.  Float64 with one rounding per operation; sine and cosine are the harmonics call's
 * own (no library); every test is a comparison, false for NaN:
 *   signals  grnet_gait_regularity's, the same bits at the same sigma: x.  y: x differenced `derivative` times (1: SPARC is defined on a speed
 *            profile), grnet_gait_entropy's, NaN where a frame it reads does not count.
 *   segments grnet_gait_spectrum's on the validity of y: `segment` = L (even, 8 .. 256), `hop`, candidates, used (0 below min_segments).  A
 *            sequence of T frames has slots = (T - L) / hop + 1 slots (0 where T < L), the most it can hold; the slots of the sequences lie back to
 *            back (grnet_gait_smoothness_slots gives the prefix sums).  Nothing is capped or truncated.
 *   M_k      of one segment, no mean taken off and no window: C = sum y_i cos(2 pi k i / N), S = sum y_i sin(..) in rising i from +0.0, nfft = N
 *            (even, L .. 4096), the table indexed by (k i) mod N; M_k = sqrt(C C + S S) for k = 0 .. k_c, the largest k with (k fps) / N <= f_cut
 *            (0 < f_cut <= fps / 2).  M_max: the largest, at the smallest k of a tie (peak_bin).  Not positive and finite: the row is NaN behind start.
 *   sparc    m_k = M_k / M_max; k_first, k_last the first and the last k with m_k >= amplitude (in (0, 1]); u = 1 / (k_last - k_first);
 *            sparc = 0 - sum_{k_first <= k < k_last} sqrt(u u + (m_(k+1) - m_k)^2) in rising k from +0.0; 0.0 where k_first = k_last.
 *   dj       on x of the same L frames: v_i = x_(i+1) - x_i, j_i = ((x_(i+3) - 3 x_(i+2)) + 3 x_(i+1)) - x_i, v_peak = max |v_i|,
 *            dj = ((sum j_i j_i) (L - 1)^3) / (v_peak v_peak), NaN where v_peak is not positive.  fps cancels.  THE LOGARITHM IS THE CALLER'S:
 *            ldlj = -ln(dj) is taken on the host (as the Python layer does).
 *   row      n (valid y), candidates, used, defined (segments with a finite sparc), sparc_mean, sparc_sd (sqrt(sum d^2 / defined)), sparc_min,
 *            sparc_max, last_hz_mean (the mean of (k_last fps) / N), dj_defined; NaN behind used where used is 0.
 * per_frame_dev (sum T, 4) float64.  per_segment_dev (sum slots, 4, 8) float64: start, sparc, k_first, k_last, peak_bin, peak_magnitude, dj, v_peak;
 * NaN everywhere behind the candidates; written whatever used is; may be null where there is no slot.  per_seq_dev (n_seq, 4, 10) float64.
 * A wave per (sequence, channel) lays the segments; a workgroup per (slot, channel), a lane per bin, makes a row; a wave per (sequence, channel)
 * reads the sequence's row off them; no atomics; across lanes only a maximum, a first and a last index are joined: a sequence's outputs have the same
 * bits alone or among others.  Needs no weights.  At most five launches (four with sigma = 0) behind one small copy from pinned memory; no host
 * synchronisation; the scratch is the box calls'.
 * GRNET_EINVAL (with a message, nothing is launched, the outputs stay untouched): a null required pointer, J < 1, a table index outside [0, J), n_seq
 * outside [1, 8192], frame_offsets[0] != 0, offsets that do not increase, a sequence of more than 32768 frames, sigma outside [0, 16], fps not
 * positive and finite, derivative outside [0, 2], segment odd or outside [8, 256], hop outside [segment / 8, segment], min_segments outside
 * [1, 2^20], nfft odd or outside [segment, 4096], not 0 < f_cut <= fps / 2, amplitude outside (0, 1].  Nothing is refused on the data.
 * grnet_op_gait_sparc: y, the segments and the rows alone (test hook) on signals_dev float64 (sum T, 4).
 * grnet_gait_smoothness_slots: host only, no handle: slots_host[q] = the slots in front of sequence q, slots_host[n_seq] all of them; GRNET_EINVAL
 * for a null pointer, n_seq < 1, offsets that do not increase from 0, segment or hop outside their limits. */
int grnet_gait_smoothness(grnet_t* h, const float* joints3d_dev, int J, const int32_t* frame_offsets_host, int n_seq, const int32_t* joints_host,
                          const double* trans_dev, const int32_t* exclude_dev, double fps, double sigma, int derivative, int segment, int hop, int nfft,
                          double f_cut, double amplitude, int min_segments, double* per_frame_dev, double* per_segment_dev, double* per_seq_dev, void* stream);
int grnet_op_gait_sparc(grnet_t* h, const double* signals_dev, const int32_t* exclude_dev, const int32_t* frame_offsets_host, int n_seq, double fps,
                        int derivative, int segment, int hop, int nfft, double f_cut, double amplitude, int min_segments, double* per_segment_dev,
                        double* per_seq_dev, void* stream);
int grnet_gait_smoothness_slots(const int32_t* frame_offsets_host, int n_seq, int segment, int hop, int64_t* slots_host);

/* Recurrence quantification of the same four body signals (Webber and Zbilut 1994; Marwan et al. 2007; on gait Labini et al. 2012 and Riva et al.
 * 2013 -- on a trunk sensor over minutes of walking; these signals are joint positions of a pose model over some 15 strides, the radius rule is this
 * project's and the defaults are unvalidated on its output): every pair of points of the delay-embedded signal against one radius, and the runs of
 * recurrent pairs along each diagonal counted by their length (which is the specification).  joints3d_dev, frame_offsets_host,
 * joints_host, trans_dev and exclude_dev as grnet_gait_regularity takes them.  Float64 with one rounding per operation; every test is a comparison,
 * false for NaN:
 *   signals  grnet_gait_regularity's, the same bits at the same sigma.  A frame counts for a channel where its signal is finite and exclude is 0.
 *   y        grnet_gait_entropy's: the signal differenced `derivative` times (1, velocities, as grnet_gait_stability), NaN where invalid.
 *   spread   grnet_gait_entropy's n, mu, SD over the valid y, r = radius SD; eps2 = (r r) dim.  Where r is not > 0 nothing is recurrent.
 *   points   grnet_gait_stability's: span = (dim - 1) lag, M = T - span points, valid iff their dim values all are; points = the valid ones.
 *   pairs    i < j < M with j - i > theiler; comparable iff both points are valid; recurrent iff comparable and D2(i, j) <= eps2, D2 as
 *            grnet_gait_stability adds it, no square root.  An infinite D2 is comparable and not recurrent.
 *   lines    on diagonal s = j - i, theiler < s < M, in rising i: a maximal run of consecutive recurrent pairs is a line of its length; a pair that
 *            is not recurrent or not comparable ends it; a line at an end of the diagonal counts with the length it has (no border correction).
 * per_frame_dev (sum T, 4) float64.  per_seq_dev (n_seq, 4, 5) float64: [n, mean, sd, r, eps2].  hist_dev (n_seq, 4, 255) int64: hist[l - 1] lines of
 * length l = 1 .. 255.  counts_dev (n_seq, 4, 6) int64: [points, comparable, recurrent, long_lines (l >= 256), long_points (the sum of their
 * lengths), longest (0 with no line)].  Always sum l hist[l - 1] + long_points = recurrent.  THE LINE THRESHOLD AND THE LOGARITHM ARE THE CALLER'S
 * (INTEGRATION.md states the formulas; the Python layer's pipeline.recurrence_rows takes lines of min_line = 2 and more where points >= 50).
 * A workgroup per (sequence, channel, part of up to 16), a lane per circular offset, the signal in LDS; line ends go into an LDS histogram by integer
 * atomic adds, the only atomics: no global and no floating-point atomics, so a sequence's outputs have the same bits alone or among others.  Then a
 * workgroup per (sequence, channel) adds the parts in part order.  The work is QUADRATIC in a sequence's frames.  Needs no weights.  At most five
 * launches (four with sigma = 0) behind one small copy from pinned memory; no host synchronisation; the scratch is the box calls'.
 * GRNET_EINVAL (with a message, nothing is launched, the outputs stay untouched): a null required pointer, J < 1, a table index outside [0, J), n_seq
 * outside [1, 8192], frame_offsets[0] != 0, offsets that do not increase, a sequence of more than 32768 frames, sigma outside [0, 16], derivative
 * outside [0, 2], dim outside [2, 8], lag outside [1, 16], theiler outside [0, 4096], radius not finite or outside (0, 10].  Nothing is refused on the
 * data.
 * grnet_op_gait_recurrence_counts: y, the spread, the pairs and the rows alone (test hook) on signals_dev float64 (sum T, 4). */
int grnet_gait_recurrence(grnet_t* h, const float* joints3d_dev, int J, const int32_t* frame_offsets_host, int n_seq, const int32_t* joints_host,
                          const double* trans_dev, const int32_t* exclude_dev, double sigma, int derivative, int dim, int lag, int theiler, double radius,
                          double* per_frame_dev, double* per_seq_dev, int64_t* hist_dev, int64_t* counts_dev, void* stream);
int grnet_op_gait_recurrence_counts(grnet_t* h, const double* signals_dev, const int32_t* exclude_dev, const int32_t* frame_offsets_host, int n_seq,
                                    int derivative, int dim, int lag, int theiler, double radius, double* per_seq_dev, int64_t* hist_dev,
                                    int64_t* counts_dev, void* stream);

/* Inference.__getitem__ -- lib/dataset/inference.py:71-87 (get_single_image_crop_demo + ToTensor + Normalize,
 * lib/data_utils/img_utils.py:252-285,355-363; rot = 0): n uint8 HWC frames (n,H,W,3) [one_image_for_all: a single
 * (H,W,3) frame shared by all boxes] and boxes (n,4) [cx,cy,w,h] -> (n,3,224,224) fp32 normalised crops, all device
 * pointers.  `scale` multiplies w,h (the reference applies its bbox scale here a second time). */
int grnet_crop_normalise(grnet_t* h, const unsigned char* images_dev, int n, int height, int width, int one_image_for_all,
                         const float* bboxes_dev, float scale, int bgr, float* out_dev, void* stream);

/* The same step with OpenCV's OWN arithmetic -- cv2.warpAffine(img, trans, (224,224), INTER_LINEAR, BORDER_CONSTANT) as
 * generate_patch_image_cv calls it (lib/data_utils/img_utils.py:90-113): positions in 1/32-pixel fixed point from the inverse
 * affine map (AB_BITS 10, INTER_BITS 5, round half to even), 15-bit blending weights, taps outside the image 0, then ToTensor +
 * Normalize (:355-363).  inv_affine_dev: (n,6) float64, the inverse of `trans` per frame, which the HOST computes the way
 * gen_trans_from_patch_cv (:54-88: float32 triangle points), cv2.getAffineTransform (6x6 solve in double) and warpAffine's own
 * inversion do -- pipeline.cv_inverse_affine.  This is the default crop of demo.py / batch_generation.py; grnet_crop_normalise
 * (exact bilinear in float) stays for A/B.  cv2 is absent offline: agreement with a real OpenCV build is argued from its source
 * (DESIGN.md), the uint8 patch is bit-identical to the oracle's restatement of the same arithmetic. */
int grnet_crop_normalise_cv(grnet_t* h, const unsigned char* images_dev, int n, int height, int width, int one_image_for_all,
                            const double* inv_affine_dev, int bgr, float* out_dev, void* stream);
/* The same for ANY box, as generate_patch_image_cv crops it (lib/data_utils/img_utils.py:90-113): maps_dev is (n,10) float64 --
 * [0..5] the inverse affine map of the (first) warp, [6] iw, [7] ih, [8] tx, [9] ty.  iw = 0: a square box, one warp, as above.
 * iw > 0: bb_width != bb_height (:97-106) -- the first warp resizes the scaled box, aspect kept, to an iw x ih 8-bit image
 * (iw, ih = int(s*w), int(s*h), s = 224 / max(w, h)), a second warpAffine moves it by (224/2 - iw/2, 224/2 - ih/2) into the patch;
 * (tx, ty) is the inverse translation.  Same fixed-point arithmetic for both warps, the intermediate image rounded to 8 bits as
 * OpenCV returns it (it is computed on the fly, never stored).  The host forms the records: pipeline.cv_crop_maps.  This is the crop
 * GRNet.crop_normalise / demo.py / batch_generation.py use. */
int grnet_crop_normalise_cv_maps(grnet_t* h, const unsigned char* images_dev, int n, int height, int width, int one_image_for_all,
                                 const double* maps_dev, int bgr, float* out_dev, void* stream);

/* Copy a named intermediate of the LAST forward (first n_frames images) into out_dev as a dense
 * (n,C,H,W) tensor; shape_out[3] receives C,H,W (out_dev may be NULL to query the shape).  Names:
 * stem_conv1, stem_conv2, layer1, layer1.{0..3}, layer1.{0..3}.{conv1,conv2}, layer1.0.downsample (unless the bf16 plan merges it into conv3),
 * transition1.{0,1}, transition2.2, transition3.3, stage{2,3,4}.{branch},
 * up{2,3,4}.{layer}.{bilinear,conv}, cat (the 480-channel backbone output), head.{first,part_feats,heat,smpl_feats,cam_shape}
 * (head.first: the two 480 -> 128 first convolutions side by side), and per HR module stage{2,3,4}.{module}.x{branch} (the branch
 * outputs = the fuse layer's inputs) / .y{branch} (the module's outputs) / .b{branch}.{block}.conv1 (a BasicBlock's first convolution) /
 * .b{branch}.{block} (its output; block 3's is .x{branch}) / fp32 handles only: .d{i}.{j}.{level}, the output of stride-2 convolution
 * `level` of the fuse layer's down chain from branch j to output i (the first links of the chains from one branch are one launch: one
 * name per slice; the chain (nb-1, nb-2) is the convolution that finishes output nb-1 and has no such name).  Parity tests compare these
 * with the oracle's taps of hrnet.py:469-536 and pare.py:305-336.
 * GRNET_EINVAL if n_frames is outside [1, frames of the last forward] (nothing is copied); GRNET_ESTATE if the last forward did not
 * write the tensor to memory (bf16, large calls: a convolution inside a row-walking or chain launch other than its last one, e.g.
 * stem_conv1 from 64 frames on) -- the buffer would hold an earlier forward's values; GRNET_ESTATE as well on a compact-arena handle
 * (grnet_create_ex) for every tensor a later one of the forward is placed over. */
int grnet_debug_tensor(grnet_t* h, const char* name, int n_frames, float* out_dev, int64_t* shape_out, void* stream);

/* ---- the exchange: all-gather of the per-frame records of a sharded clip (SURVEY 8b `grnet_allgather`, 8e) -------------------------------------
 * The reference has no counterpart (demo.py:126-188 and batch_generation.py:289-329 are one process on one device).  One process per GPU; every
 * rank runs grnet_forward on its contiguous frame range with the output pointers aimed INTO its send block, then ONE grnet_allgather (RCCL
 * ncclAllGather over xGMI, enqueued on `stream` like every other call) reassembles the sequence on every rank before anything temporal runs.
 * RCCL is looked up at run time (librccl.so.1, the copy the process already holds if any): the library loads and runs on one GPU without it, the
 * grnet_comm_* calls then fail with GRNET_ESTATE.  Bootstrap: rank 0 calls grnet_comm_unique_id and hands the 128 bytes to the other ranks over any host
 * channel (the launcher's store, a file, MPI); all ranks then call grnet_comm_create together (it blocks until every rank has arrived).
 * A host that already owns an ncclComm_t passes it to grnet_comm_adopt instead (not destroyed by grnet_comm_destroy).
 * Errors of this group: grnet_comm_last_error() (per thread), since no grnet_t is involved. */
typedef struct grnet_comm grnet_comm_t;
#define GRNET_COMM_ID_BYTES 128
/* Local and non-collective: 0 when RCCL could be bound in this process (librccl.so.1, or the one library named by the environment variable
 * GRNET_RCCL_LIB), GRNET_ESTATE otherwise.  Every rank calls it FIRST and the ranks agree on the minimum over a host channel before any of them
 * enters grnet_comm_unique_id / grnet_comm_create, so that no rank waits inside a collective the others never enter. */
int grnet_comm_probe(void);
int grnet_comm_unique_id(void* id_out, int id_size /* >= GRNET_COMM_ID_BYTES */);
int grnet_comm_create(grnet_comm_t** out_comm, const void* id, int world, int rank, int device_id);
int grnet_comm_adopt(grnet_comm_t** out_comm, void* nccl_comm /* ncclComm_t */, int world, int rank);
/* recv_dev holds world * bytes_per_rank bytes; rank r's block lands at offset r * bytes_per_rank (send_dev may alias its own slot). */
int grnet_allgather(grnet_comm_t* comm, const void* send_dev, void* recv_dev, size_t bytes_per_rank, void* stream);
int grnet_comm_info(grnet_comm_t* comm, int* world, int* rank);
void grnet_comm_destroy(grnet_comm_t* comm);
const char* grnet_comm_last_error(void);

const char* grnet_last_error(grnet_t* h);
const char* grnet_version(void);
void grnet_destroy(grnet_t* h);

#ifdef __cplusplus
}
#endif
#endif /* GRNET_HIP_H */
