"""ctypes binding of libgrnet_hip.so (the C ABI declared in include/grnet_hip.h).

The product path has NO fallback: if the HIP library is missing or fails to load, importing the
model raises.  Nothing here touches ``oracle/``.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# GRNET_LIB_PATH: a diagnostic build of the same library (make ABLATION=1 BUILD=build_abl LIB=../libgrnet_hip_abl.so), tools/ only
LIB_PATH = os.environ.get("GRNET_LIB_PATH") or os.path.join(_HERE, "libgrnet_hip.so")

OK, EINVAL, ENOENT, ENOMEM, EHIP, ESTATE = 0, -22, -2, -12, -5, -1
DTYPE_F32, DTYPE_I64 = 0, 1
PRECISION_F32, PRECISION_BF16 = 0, 1
CREATE_COMPACT_ARENA = 1
JOINT_REGRESSOR_MAX_ROWS = 64
JOINTS_SPIN49, JOINTS_SPIN2, JOINTS_KINECTV2 = 0, 1, 2
PLAN_COUNTS = ("ops", "waits_all", "records_all", "waits", "records", "lanes_all", "lanes_joined")     # the GRNET_PLAN_* enumerators, in order
RASTER_MAX_DIM, RASTER_SLOTS = 4096, 16
SEG_MAX_POINTS, SEG_MAX_SEGMENTS, SEG_MAX_WIDTH = 1024, 4096, 16
BBOX_MAX_JOINTS, BBOX_MAX_FRAMES, MEDOID_MAX_SPLITS = 64, 4096, 64
METRIC_MAX_JOINTS = 64
TRANS_MAX_PAIRS = 64
TRACK_PAD = {"zero": 0, "edge": 1}
GAIT_JOINTS_KINECTV2 = (0, 20, 12, 16, 14, 18, 15, 19)         # pelvis, spine-shoulder, left hip, right hip, left ankle, right ankle, left foot, right foot
# pelvis, spine-shoulder, then left and right hip, knee, ankle, foot, shoulder, elbow, wrist
KINEMATICS_JOINTS_KINECTV2 = (0, 20, 12, 16, 13, 17, 14, 18, 15, 19, 4, 8, 5, 9, 6, 10)
# (proximal joint, distal joint, mass, the COM's fraction from the proximal joint): Winter's whole-body fractions laid on the kinectv2 joints --
# trunk, head and neck, then left and right upper arm, forearm, hand, thigh, shank, foot.  The layout is this project's choice and unvalidated.
BALANCE_SEGMENTS_KINECTV2 = ((0, 20, 0.497, 0.5), (20, 3, 0.081, 1.0), (4, 5, 0.028, 0.436), (8, 9, 0.028, 0.436), (5, 6, 0.016, 0.430), (9, 10, 0.016, 0.430),
                             (6, 7, 0.006, 0.506), (10, 11, 0.006, 0.506), (12, 13, 0.100, 0.433), (16, 17, 0.100, 0.433), (13, 14, 0.0465, 0.433),
                             (17, 18, 0.0465, 0.433), (14, 15, 0.0145, 0.5), (18, 19, 0.0145, 0.5))
OPT_USE_GRAPH, OPT_CONV_TILE, OPT_MULTI_LANE, OPT_WINOGRAD, OPT_BF16_CHAIN, OPT_GRU_MODE, OPT_BF16_MIN_FRAMES = 1, 2, 3, 7, 8, 9, 10


class Outputs(C.Structure):
    """grnet_outputs_t"""
    _fields_ = [(n, C.c_void_p) for n in (
        "theta", "verts", "kp_2d", "kp_3d", "rotmat", "point_local_feat", "cam_shape_feats", "pred_rot6d",
        "features", "part_attn", "smpl_feats")]


class GaitOutputs(C.Structure):
    """grnet_gait_outputs_t"""
    _fields_ = [(n, C.c_void_p) for n in ("pred_avg", "pred_phase", "pred_cparam", "point_local_feat")]


EXPORTS = {
    "grnet_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int]),
    "grnet_create_ex": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_uint]),
    "grnet_arena_query": (C.c_int, [C.c_int, C.c_int, C.c_uint, C.POINTER(C.c_int64)]),
    "grnet_arena_layout": (C.c_int, [C.c_int, C.c_int, C.c_uint, C.c_char_p, C.c_int]),
    "grnet_arena_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "grnet_arena_fill": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "grnet_arena_assign": (C.c_int, [C.c_int, C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int64),
                                     C.POINTER(C.c_int64)]),
    "grnet_load_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.c_int]),
    "grnet_load_smpl": (C.c_int, [C.c_void_p] + [C.c_void_p] * 7),
    "grnet_finalize_weights": (C.c_int, [C.c_void_p]),
    "grnet_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(Outputs), C.c_void_p]),
    "grnet_gru_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    "grnet_tsattn_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "grnet_tsattn_plan": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32)]),
    "grnet_temporal_taps": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "grnet_temporal_tap_layout": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "grnet_set_option": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "grnet_tune": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "grnet_get_tuning": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_int]),
    "grnet_set_tuning": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p]),
    "grnet_num_kernel_launches": (C.c_int, [C.c_void_p]),
    "grnet_plan_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "grnet_num_conv_launches": (C.c_int, [C.c_void_p]),
    "grnet_conv_flops_per_frame": (C.c_double, [C.c_void_p]),
    "grnet_conv_executed_flops_per_frame": (C.c_double, [C.c_void_p]),
    "grnet_describe_conv": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_char_p, C.c_int]),
    "grnet_describe_conv_macs": (C.c_double, [C.c_void_p, C.c_int]),
    "grnet_conv_executed_flops_per_frame_n": (C.c_double, [C.c_void_p, C.c_int]),
    "grnet_conv_kernel_info": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_double)]),
    "grnet_time_conv": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_float)]),
    "grnet_conv_launch_form": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int)]),
    "grnet_op_timeline": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_char_p, C.c_int]),
    "grnet_time_convs": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_float)]),
    "grnet_op_conv2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "grnet_op_conv2d_adds": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                       C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                       C.POINTER(C.c_int), C.c_void_p, C.c_int, C.c_void_p]),
    "grnet_op_conv_chain": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                      C.POINTER(C.c_float), C.c_void_p]),
    "grnet_op_bilinear2x": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "grnet_op_attention_pool": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grnet_smpl_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "grnet_crop_normalise": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_int,
                                       C.c_void_p, C.c_void_p]),
    "grnet_crop_normalise_cv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                          C.c_void_p]),
    "grnet_crop_normalise_cv_maps": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                          C.c_void_p]),
    "grnet_head_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(Outputs), C.c_void_p]),
    "grnet_gait_correct": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                     C.POINTER(Outputs), C.POINTER(GaitOutputs), C.c_void_p]),
    "grnet_set_joint_regressor": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_int]),
    "grnet_joint_regressor_rows": (C.c_int, [C.c_void_p]),
    "grnet_regress_joints": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "grnet_op_rot6d_to_rotmat": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "grnet_op_rotmat_to_aa": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "grnet_op_aa_to_rotmat": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "grnet_op_one_euro": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "grnet_smooth_pose": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    "grnet_load_faces": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "grnet_render_meshes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                      C.c_int, C.c_void_p]),
    "grnet_render_meshes_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                         C.c_int, C.c_uint, C.c_void_p]),
    "grnet_op_raster_setup": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    "grnet_op_raster": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "grnet_op_raster_lines": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "grnet_spin_joints": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "grnet_render_segments": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "grnet_op_segments_setup": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "grnet_op_raster_segments": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                           C.c_void_p]),
    "grnet_bbox_from_joints2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grnet_op_medoid": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grnet_pose_metrics": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), C.c_int,
                                     C.POINTER(C.c_int32), C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "grnet_fit_translation": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32),
                                        C.c_int, C.POINTER(C.c_double), C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grnet_track_boxes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_double, C.c_int, C.c_double, C.c_int, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "grnet_op_median1d": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "grnet_op_gauss1d": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_double, C.c_void_p, C.c_void_p]),
    "grnet_gait_parameters": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), C.c_void_p, C.c_double, C.c_double,
                                        C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grnet_op_gait_events": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p]),
    "grnet_gait_kinematics": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), C.c_void_p, C.c_double, C.c_int, C.c_int,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grnet_op_gait_cycles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grnet_gait_turns": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_double, C.c_double,
                                   C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grnet_op_gait_turn_runs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
                                          C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grnet_gait_contacts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), C.c_void_p, C.c_double, C.c_double, C.c_double,
                                      C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grnet_op_gait_contact_runs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int,
                                             C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grnet_gait_regularity": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_double, C.c_double,
                                        C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grnet_op_gait_autocorr": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_double, C.c_int, C.c_int, C.c_double, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "grnet_gait_harmonics": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "grnet_op_gait_stride_dft": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_double, C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grnet_gait_entropy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_double, C.c_int,
                                     C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grnet_op_gait_sampen": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "grnet_gait_stability": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_double, C.c_int,
                                       C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grnet_op_gait_divergence": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    "grnet_gait_spectrum": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_double, C.c_double,
                                      C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grnet_op_gait_welch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                      C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grnet_gait_smoothness": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_double, C.c_double,
                                        C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grnet_op_gait_sparc": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                      C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grnet_gait_smoothness_slots": (C.c_int, [C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    "grnet_gait_recurrence": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_double, C.c_int,
                                        C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grnet_op_gait_recurrence_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grnet_gait_coordination": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), C.c_void_p, C.c_double, C.c_double, C.c_int,
                                          C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "grnet_op_gait_cross_welch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                            C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grnet_gait_balance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), C.c_void_p, C.POINTER(C.c_int32),
                                     C.POINTER(C.c_double), C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "grnet_op_gait_balance_steps": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int,
                                              C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grnet_gait_balance_com": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_double,
                                         C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grnet_mesh_moments": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grnet_op_mesh_moments": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "grnet_faces_closed": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "grnet_gait_step_tables": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "grnet_bootstrap_table": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_uint64,
                                        C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grnet_op_procrustes":(C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "grnet_debug_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]),
    "grnet_comm_probe": (C.c_int, []),
    "grnet_comm_unique_id": (C.c_int, [C.c_void_p, C.c_int]),
    "grnet_comm_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "grnet_comm_adopt": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_int]),
    "grnet_allgather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "grnet_comm_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "grnet_comm_destroy": (None, [C.c_void_p]),
    "grnet_comm_last_error": (C.c_char_p, []),
    "grnet_last_error": (C.c_char_p, [C.c_void_p]),
    "grnet_version": (C.c_char_p, []),
    "grnet_destroy": (None, [C.c_void_p]),
}

_lib = None


def load():
    """Load the shared library once; raise loudly if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own HIP runtime under the same SONAMEs as /opt/rocm's: import it FIRST so that
    # this library binds to the runtime torch allocates tensors with (one runtime per process).
    import torch  # noqa: F401
    if not os.path.isfile(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C video-based-gait-analysis-for-dementia_amd/csrc`). There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in EXPORTS.items():
        fn = getattr(lib, name)          # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class GrnetError(RuntimeError):
    pass


COMM_ID_BYTES = 128


def check_comm(lib, rc, what):
    if rc != 0:
        raise GrnetError(f"{what} failed with code {rc}: {lib.grnet_comm_last_error().decode()}")


def check(lib, handle, rc, what):
    if rc != 0:
        msg = lib.grnet_last_error(handle).decode() if handle else ""
        raise GrnetError(f"{what} failed with code {rc}: {msg}")
