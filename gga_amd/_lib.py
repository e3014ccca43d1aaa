"""ctypes binding of ``libgga_hip.so`` (the C ABI declared in include/gga_hip.h).

The library is built in-tree by ``gga_amd/csrc/Makefile`` (``__graft_entry__.build()``)
and is the *only* compute path of the product: there is no CPU fallback. Loading
fails loudly when the shared object is missing, and every entry point raises
``RuntimeError`` with ``gga_last_error()`` on a non-zero status.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libgga_hip.so')
ABI_VERSION = 37

_lib = None

vp, i32, i64, f32, sz = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t
I3 = C.POINTER(C.c_int32 * 3)


class VoxelParams(C.Structure):
    _fields_ = [('voxel_size', C.c_float * 3), ('pc_range', C.c_float * 6),
                ('max_points', C.c_int32), ('max_voxels', C.c_int32)]


PFN_SAVED_DOUBLES = 239     # PFN_SAVED_ROWS + 1


class PfnParams(C.Structure):
    _fields_ = [('voxel_size', C.c_float * 3), ('offsets', C.c_float * 3), ('eps', C.c_float),
                ('momentum', C.c_float), ('training', C.c_int32), ('in_features', C.c_int32),
                ('channels', C.c_int32)]


MAX_TASKS = 8      # GGA_MAX_TASKS


class Task(C.Structure):
    """gga_task: one task's pointers for the loss kernels (a stage reads only its own fields)."""
    _fields_ = [('logits', vp), ('target', vp), ('n_heat', i64), ('focal_out', vp), ('focal_grad', vp), ('grad_logits', vp),
                ('reg', vp), ('height', vp), ('dim', vp), ('rot', vp), ('g_reg', vp), ('g_height', vp), ('g_dim', vp),
                ('g_rot', vp), ('ind', vp), ('mask', vp), ('pred', vp), ('grad_pred', vp), ('anno_box', vp), ('lidar2img', vp),
                ('bound_mask', vp), ('ibp_xy', vp), ('ibp_offsets', vp), ('ibp_slot', vp), ('n_ibp_obj', C.c_int32),
                ('losses', vp), ('box_out', vp), ('term_grads', vp), ('grad_losses', vp)]


class TaskTable(C.Structure):
    _fields_ = [('n_tasks', C.c_int32), ('task', Task * MAX_TASKS)]


MULTICLASS_NMS_MAX_CLASSES = 128    # GGA_MULTICLASS_NMS_MAX_CLASSES
TTA_MAX_VIEWS = 16                  # GGA_TTA_MAX_VIEWS
TTA_MAX_MAPS = MAX_TASKS * 6        # GGA_TTA_MAX_MAPS
TTA_PLAIN, TTA_REG, TTA_ROT, TTA_VEL = range(4)


class TtaMap(C.Structure):
    _fields_ = [('src', vp), ('dst', vp), ('channels', C.c_int32), ('kind', C.c_int32)]


class TtaTable(C.Structure):
    """gga_tta_table: the views' scale groups and flips, and one entry per head map."""
    _fields_ = [('n_maps', C.c_int32), ('n_views', C.c_int32), ('n_groups', C.c_int32), ('group', C.c_int32 * TTA_MAX_VIEWS),
                ('hflip', C.c_int32 * TTA_MAX_VIEWS), ('vflip', C.c_int32 * TTA_MAX_VIEWS), ('map', TtaMap * TTA_MAX_MAPS)]


MONO3D_TTA_MAX_MAPS = 48            # GGA_MONO3D_TTA_MAX_MAPS
MONO3D_TTA_MEAN, MONO3D_TTA_REG = range(2)
MONO3D_COLLECT_MAX_IMAGES = 4096    # GGA_MONO3D_COLLECT_MAX_IMAGES


class Mono3dTtaMap(C.Structure):
    _fields_ = [('src', vp), ('dst', vp), ('channels', C.c_int32), ('H', C.c_int32), ('W', C.c_int32), ('kind', C.c_int32)]


class Mono3dTtaTable(C.Structure):
    """gga_mono3d_tta_table: one entry per (output group, FPN level) of the two-view head output."""
    _fields_ = [('n_maps', C.c_int32), ('n_frames', C.c_int32), ('map', Mono3dTtaMap * MONO3D_TTA_MAX_MAPS)]


IMAGE_BATCH_MAX = 64                # GGA_IMAGE_BATCH_MAX


class ImageDesc(C.Structure):
    """gga_image_desc: where one image of a batch lies in the source buffer, its size there and in the output, its flip."""
    _fields_ = [('src_offset', C.c_int64), ('src_h', C.c_int32), ('src_w', C.c_int32), ('dst_h', C.c_int32), ('dst_w', C.c_int32),
                ('flip', C.c_int32), ('reserved', C.c_int32)]


CENTER_MAX_CLASSES = 64     # GGA_CENTER_MAX_CLASSES
CENTER_MAX_K = 512          # GGA_CENTER_MAX_K


class CenterParams(C.Structure):
    """gga_center_params: the train_cfg numbers and the class -> (task, index) table of gga_center_targets."""
    _fields_ = [('pc_range', C.c_float * 2), ('voxel_size', C.c_float * 2), ('out_size_factor', C.c_float),
                ('gaussian_overlap', C.c_float), ('min_radius', C.c_int32), ('K', C.c_int32), ('H', C.c_int32), ('W', C.c_int32),
                ('n_tasks', C.c_int32), ('n_classes', C.c_int32), ('task_classes', C.c_int32 * MAX_TASKS),
                ('task_class_base', C.c_int32 * MAX_TASKS), ('class_task', C.c_int32 * CENTER_MAX_CLASSES),
                ('class_index', C.c_int32 * CENTER_MAX_CLASSES)]


class CenterLossTask(C.Structure):
    _fields_ = [('pred', vp), ('anno_box', vp), ('mask', vp), ('loss', vp), ('grad_loss', vp), ('grad_pred', vp)]


class CenterLossTable(C.Structure):
    _fields_ = [('n_tasks', C.c_int32), ('task', CenterLossTask * MAX_TASKS)]


class CenterLossWeights(C.Structure):
    _fields_ = [('code_weights', C.c_float * 8), ('loss_weight', C.c_float)]


FPS_REGISTER_MAX_N = 20480  # GGA_FPS_REGISTER_MAX_N
GROUP_MAX_SAMPLES = 256     # GGA_GROUP_MAX_SAMPLES
ANCHOR_MAX_GROUPS = 16      # GGA_ANCHOR_MAX_GROUPS
ANCHOR_LOSS_WORKSPACE_BYTES = 24576      # GGA_ANCHOR_LOSS_WORKSPACE_BYTES


class AnchorParams(C.Structure):
    """gga_anchor_params: the assigners' thresholds per anchor-size group and the head's target options."""
    _fields_ = [('n_groups', C.c_int32), ('n_rot', C.c_int32), ('num_classes', C.c_int32), ('assign_per_class', C.c_int32),
                ('pos_iou_thr', C.c_float * ANCHOR_MAX_GROUPS), ('neg_iou_thr', C.c_float * ANCHOR_MAX_GROUPS),
                ('min_pos_iou', C.c_float * ANCHOR_MAX_GROUPS), ('pos_weight', C.c_float), ('dir_offset', C.c_float),
                ('dir_limit_offset', C.c_float)]


class AnchorLossParams(C.Structure):
    """gga_anchor_loss_params: shapes, the (batch, channel, pixel) strides of the three prediction maps, loss constants."""
    _fields_ = [('B', C.c_int32), ('HW', C.c_int32), ('n_anchors', C.c_int32), ('num_classes', C.c_int32),
                ('diff_rad_by_sin', C.c_int32), ('reserved', C.c_int32), ('cls_stride', C.c_int64 * 3),
                ('reg_stride', C.c_int64 * 3), ('dir_stride', C.c_int64 * 3), ('gamma', C.c_float), ('alpha', C.c_float),
                ('beta', C.c_float), ('code_weight', C.c_float * 7), ('loss_weight', C.c_float * 3)]


class LossParams(C.Structure):
    _fields_ = [('B', C.c_int32), ('K', C.c_int32), ('fm_w', C.c_int32),
                ('voxel_size', C.c_float * 2), ('out_size_factor', C.c_float),
                ('pc_range', C.c_float * 2), ('code_weights', C.c_float * 5),
                ('l1_loss_weight', C.c_float), ('w_bpl', C.c_float), ('w_srl', C.c_float),
                ('w_pal', C.c_float)]


# name -> (restype, argtypes); every symbol include/gga_hip.h declares
SIGNATURES = {
    'gga_last_error': (C.c_char_p, []),
    'gga_abi_version': (i32, []),
    'gga_timing_begin': (i32, [i32, i32, i64]),
    'gga_timing_collect': (i32, [i32, vp, i32]),
    'gga_voxel_grid_size': (None, [C.POINTER(VoxelParams), C.POINTER(C.c_int32 * 3)]),
    'gga_hard_voxelize_workspace_bytes': (sz, [i32, i64]),
    'gga_hard_voxelize_batch': (i32, [vp, i32, C.POINTER(C.c_int64), vp, i32, C.POINTER(VoxelParams),
                                       vp, vp, vp, vp, vp, sz, vp]),
    'gga_dynamic_voxelize': (i32, [vp, i32, C.POINTER(C.c_int64), vp, i32, C.POINTER(VoxelParams), vp, vp, vp]),
    'gga_dynamic_voxel_map_workspace_bytes': (sz, [i64]),
    'gga_dynamic_voxel_map': (i32, [vp, vp, i32, i64, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, sz, vp]),
    'gga_dynamic_scatter_chunk': (i32, []),
    'gga_dynamic_scatter_workspace_bytes': (sz, [i64, i32]),
    'gga_dynamic_scatter_fwd': (i32, [vp, i32, i64, vp, vp, vp, vp, i64, i32, vp, vp, vp, sz, vp]),
    'gga_dynamic_scatter_bwd': (i32, [vp, i32, i64, vp, vp, vp, i64, i32, vp, vp]),
    'gga_dynamic_pfn_workspace_bytes': (sz, [i64]),
    'gga_dynamic_pfn_fwd': (i32, [vp, vp, i64, vp, vp, vp, vp, i64, C.POINTER(PfnParams)] + [vp] * 10 + [sz, vp]),
    'gga_dynamic_pfn_bwd': (i32, [vp, vp, i64, vp, i64, C.POINTER(PfnParams)] + [vp] * 11 + [sz, vp]),
    'gga_points_prepare_workspace_bytes': (sz, [i32, i64, i64]),
    'gga_points_prepare_batch': (i32, [vp, C.POINTER(C.c_int64), vp, C.POINTER(C.c_int64), vp, C.POINTER(C.c_int64),
                                        i32, i32, C.c_double, vp, C.POINTER(C.c_uint64), vp, vp, vp, sz, vp]),
    'gga_voxel_mean': (i32, [vp, vp, i64, i32, i32, i32, vp, vp]),
    'gga_pfn_workspace_bytes': (sz, [i64]),
    'gga_pfn_fwd': (i32, [vp, vp, vp, i64, vp, i32, C.POINTER(PfnParams), vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
    'gga_pfn_bwd': (i32, [vp, vp, vp, i64, vp, i32, C.POINTER(PfnParams), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
    'gga_pillar_scatter_map_bytes': (sz, [i32, i32, i32]),
    'gga_pillar_scatter_fwd': (i32, [vp, vp, i64, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp]),
    'gga_pillar_scatter_bwd': (i32, [vp, vp, i64, vp, i32, i32, i32, i32, i32, vp, vp]),
    'gga_pillar_conv_map': (i32, [vp, i64, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp]),
    'gga_sparse_index_bytes': (sz, [i64]),
    'gga_sparse_build_index': (i32, [vp, i64, i32, i32, i32, i32, vp, sz, vp]),
    'gga_sparse_out_index_bytes': (sz, [i64, i32]),
    'gga_sparse_out_sites_workspace_bytes': (sz, [i64, i32]),
    'gga_sparse_conv_out_sites': (i32, [vp, i64, i32, I3, I3, I3, I3, I3, vp, i64, vp, vp, sz, vp, sz, vp]),
    'gga_sparse_rulebook': (i32, [vp, i64, vp, i64, i32, I3, I3, I3, I3, I3, vp, i64, vp, i64, vp, vp, vp]),
    'gga_sparse_rowmask': (i32, [vp, i64, i32, vp, vp]),
    'gga_sparse_mask_order_workspace_bytes': (sz, [i64]),
    'gga_sparse_morton_order_workspace_bytes': (sz, [i64]),
    'gga_sparse_morton_order': (i32, [vp, i64, i32, i32, vp, vp, sz, vp]),
    'gga_sparse_mask_order': (i32, [vp, i64, i32, vp, vp, sz, vp]),
    'gga_sparse_split_weight_bytes': (sz, [i32, i32, i32]),
    'gga_sparse_conv_wgrad_workspace_bytes': (sz, [i64, i32, i32, i32]),
    'gga_dense_wgrad3x3_workspace_bytes': (sz, [i32, i32, i32, i32, i32]),
    'gga_sparse_pack_weight_planes': (i32, [vp, i32, i32, i32, i32, i32, vp, vp, vp]),
    'gga_sparse_conv_apply_tiles': (i64, [i64]),
    'gga_sparse_conv_apply_bn_bwd': (i32, [vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, vp, i64, i32, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp]),
    'gga_sparse_bev_nhwc_fwd': (i32, [vp, vp, i64, i32, i32, i32, i32, i32, vp, vp]),
    'gga_sparse_bev_nhwc_bwd': (i32, [vp, vp, i64, i32, i32, i32, i32, i32, vp, vp]),
    'gga_sparse_halo_tile_rows': (i64, []),
    'gga_sparse_halo_build': (i32, [vp, vp, i64, i64, i32, i32, vp, vp, vp, vp]),
    'gga_sparse_conv_apply_halo': (i32, [vp, vp, vp, vp, i32, vp, vp, i64, i64, i32, i32, i32, i32, vp, i64, i32, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp]),
    'gga_sparse_conv_wgrad_planes': (i32, [vp, i64, vp, i64, vp, i64, i32, i32, i32, vp, i32, vp, vp, vp, sz, vp]),
    'gga_deconv_stream_tiles': (i64, [i64, i32, i32]),
    'gga_deconv_stream_fwd': (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp]),
    'gga_deconv_stream_bwd': (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp]),
    'gga_absmax_bits': (i32, [vp, i64, i32, i64, vp, vp]),
    'gga_dense_conv3x3_pack_planes': (i32, [vp, i64, i64, i64, i64, i32, i32, i32, i32, vp, vp, vp]),
    'gga_dense_conv3x3_levels': (i32, [i32, vp, vp, vp, vp, i32, i32, i32, vp, i64, i32, vp, vp, vp, i32, i32, vp, vp]),
    'gga_dense_conv3x3_bn_bwd_pays': (i32, [i32, i32, i32, i32]),
    'gga_dense_conv3x3_bn_bwd_pays_planes': (i32, [i32, i32, i32, i32, i32]),
    'gga_dense_conv3x3_bn_bwd': (i32, [vp, vp, i32, i32, i32, i32, i32, vp, i64, i32, vp, i32, vp, vp, vp, i64, vp, vp, vp, vp, vp]),
    'gga_absmax_table_blocks': (i64, [i64]),
    'gga_absmax_table': (i32, [vp, i32, i64, vp, i32, vp]),
    'gga_pack_weights_table': (i32, [vp, i32, i64, i32, vp]),
    'gga_dense_wgrad3x3_block_amax': (i32, [vp, vp, i32, i32, i32, i32, i32, vp, i64, i64, i64, i64, i32, i32, vp, i32, vp, i32, vp, sz, vp]),
    'gga_dense_conv3x3_tile_rows': (i32, [i32, i32, i32, i32, i32]),
    'gga_dense_conv3x3_stat_rows': (i64, [i32, i32, i32, i32, i32, i32]),
    'gga_bn_relu_workspace_bytes': (sz, [i64, i32]),
    'gga_bn_relu_mask_bytes': (sz, [i64, i32]),
    'gga_bn_relu_fwd': (i32, [vp, vp, vp, vp, vp, vp, i64, i32, f32, f32, i32, i32, vp, i64, vp, vp, vp, i32, vp, vp, sz, vp]),
    'gga_bn_relu_bwd': (i32, [vp, i64, vp, vp, vp, vp, i64, i32, i32, i32, vp, vp, vp, vp, vp, vp, sz, vp]),
    'gga_column_sums': (i32, [vp, i64, i32, vp, vp, sz, vp]),
    'gga_bn_relu_bwd_partials': (i32, [vp, i64, vp, vp, vp, i64, i32, i32, vp, i32, vp, vp, vp, vp, vp, sz, vp]),
    'gga_gn_relu_workspace_bytes': (sz, [i32, i32]),
    'gga_gn_relu_fwd': (i32, [vp, vp, vp, i32, i64, i32, i32, f32, i32, vp, vp, vp, vp, vp, sz, vp]),
    'gga_gn_relu_bwd': (i32, [vp, vp, vp, vp, vp, i32, i64, i32, i32, i32, vp, vp, vp, vp, vp, sz, vp]),
    'gga_bn_stats': (i32, [vp, vp, vp, vp, vp, i64, i32, f32, f32, i32, vp, vp, vp, i32, i32, i32, vp, sz, vp]),
    'gga_head_conv3x3_fwd': (i32, [vp, i64, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp]),
    'gga_head_conv3x3_fwd_tiles': (i32, [vp, i64, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp]),
    'gga_head_cell_tiles_count': (i64, [i32, i32, i32]),
    'gga_head_cell_tiles': (i32, [vp, i32, i32, i32, i32, vp, vp]),
    'gga_head_conv3x3_workspace_bytes': (sz, [i32]),
    'gga_head_conv3x3_wgrad': (i32, [vp, i64, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, sz, vp]),
    'gga_head_tail_bwd': (i32, [vp, vp, i64, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, i64, vp, vp, vp, vp, sz, vp]),
    'gga_head_tile_activity': (i32, [vp, i32, i32, i32, i32, vp, vp]),
    'gga_head_branch_bwd_workspace_bytes': (sz, [i32, i32, i32, i32]),
    'gga_head_branch_bwd': (i32, [vp, vp, i64, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, i64, vp, vp, vp, i32, vp, sz, vp]),
    'gga_heatmap_splat': (i32, [vp, i32, i32, i32, vp, i32, vp, vp, i32, vp]),
    'gga_focal_loss_workspace_bytes': (sz, [i64, i32]),
    'gga_focal_loss_fwd': (i32, [C.POINTER(TaskTable), f32, f32, f32, vp, sz, vp]),
    'gga_focal_loss_bwd': (i32, [C.POINTER(TaskTable), f32, f32, f32, vp]),
    'gga_gather_pred_fwd': (i32, [C.POINTER(TaskTable), i32, i32, i32, i32, vp]),
    'gga_gather_pred_bwd': (i32, [C.POINTER(TaskTable), i32, i32, i32, i32, vp]),
    'gga_box_losses_workspace_bytes': (sz, [i32, i32, i32]),
    'gga_box_losses_fwd': (i32, [C.POINTER(TaskTable), C.POINTER(LossParams), vp, sz, vp]),
    'gga_box_losses_bwd': (i32, [C.POINTER(TaskTable), i32, i32, vp]),
    'gga_center_targets': (i32, [vp, vp, vp, i32, C.POINTER(CenterParams), vp, vp, vp, vp, vp, vp, i32, vp]),
    'gga_center_reg_loss_fwd': (i32, [C.POINTER(CenterLossTable), i32, i32, C.POINTER(CenterLossWeights), vp]),
    'gga_center_reg_loss_bwd': (i32, [C.POINTER(CenterLossTable), i32, i32, C.POINTER(CenterLossWeights), vp]),
    'gga_anchor_targets_workspace_bytes': (sz, [i64, i32]),
    'gga_anchor_targets': (i32, [vp, i32, C.POINTER(AnchorParams), vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
    'gga_anchor_loss_fwd': (i32, [C.POINTER(AnchorLossParams), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
    'gga_anchor_loss_bwd': (i32, [C.POINTER(AnchorLossParams), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    'gga_anchor_decode': (i32, [vp, i32, i32, vp, i32, i32, i32, vp, vp, C.POINTER(C.c_int64 * 3), vp, C.POINTER(C.c_int64 * 3), vp, vp, vp, vp]),
    'gga_box_iou_rotated': (i32, [vp, i32, vp, i32, i32, i32, vp, vp]),
    'gga_nms_rotated_workspace_bytes': (sz, [i32]),
    'gga_nms_rotated_sorted': (i32, [vp, i32, f32, i32, vp, vp, vp, sz, vp]),
    'gga_circle_nms_sorted': (i32, [vp, i32, C.c_double, i32, vp, vp, vp, sz, vp]),
    'gga_region_grow_workspace_bytes': (sz, [i64, i32]),
    'gga_region_grow': (i32, [vp, i64, i32, vp, vp, vp, i32, C.c_double, i32, vp, vp, sz, vp]),
    'gga_points_in_convex_polyhedra': (i32, [vp, i64, i32, vp, vp, i32, i32, vp, vp]),
    'gga_plane_inliers': (i32, [vp, i64, i32, vp, i32, C.c_double, vp, vp, vp]),
    'gga_frame_point_tests_workspace_bytes': (sz, [i64]),
    'gga_frame_point_tests': (i32, [vp, i64, i32, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, sz, vp]),
    'gga_image_box_match': (i32, [vp, vp, vp, vp, i32, i64, i32, vp, vp, vp, vp, vp]),
    'gga_kitti_eval_overlaps': (i32, [vp, vp, i64, vp, vp, i64, i32, i32, i32, i32, vp, vp, i64, vp]),
    'gga_kitti_eval_stats_workspace_bytes': (sz, [i32, i32, i32]),
    'gga_kitti_eval_stats': (i32, [vp, i32, vp, i64, vp, vp, vp, vp, i64, vp, i64, vp, i64, vp, vp, i32, vp, vp, i32, i32, i32, i32, i32,
                                   i32, i32, vp, vp, vp, vp, vp, vp, sz, vp]),
    'gga_kitti_format_dets': (i32, [vp, vp, vp, i64, vp, i32, vp, vp, vp, C.POINTER(C.c_float * 6), vp, vp, vp, vp, vp]),
    'gga_kitti_format_dets_cam': (i32, [vp, vp, vp, i64, vp, i32, vp, vp, vp, vp, vp, vp]),
    'gga_image_batch': (i32, [vp, i64, C.POINTER(ImageDesc), i32, vp, i32, i32, i32, i32, vp, vp]),
    'gga_indoor_eval_match': (i32, [vp, vp, i64, vp, vp, i64, i32, vp, vp, vp]),
    'gga_indoor_eval_workspace_bytes': (sz, [i64, i32]),
    'gga_indoor_eval_assign': (i32, [vp, vp, vp, vp, i64, vp, i64, i32, C.POINTER(C.c_float * 8), i32, vp, vp, sz, vp]),
    'gga_centerpoint_detect_workspace_bytes': (sz, [i32, i32]),
    'gga_centerpoint_detect': (i32, [vp, vp, vp, i32, i32, i32, i32, vp, C.c_float, i32, C.c_float, vp, C.c_float, i32, i32, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
    'gga_multiclass_nms3d_workspace_bytes': (sz, [i64, i32, i32]),
    'gga_multiclass_nms3d': (i32, [vp, vp, vp, i64, i32, i32, f32, f32, vp, vp, vp, vp, sz, vp]),
    'gga_tta_merge_maps': (i32, [C.POINTER(TtaTable), i32, i32, i32, vp]),
    'gga_mono3d_tta_merge': (i32, [C.POINTER(Mono3dTtaTable), vp]),
    'gga_mono3d_collect_workspace_bytes': (sz, [i64, i32, i32]),
    'gga_mono3d_collect': (i32, [vp, vp, vp, i32, i64, i32, vp, i32, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
    'gga_points_in_boxes': (i32, [vp, vp, i32, i32, i32, i32, vp, vp]),
    'gga_fcos3d_targets': (i32, [vp, i32, i32, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_float), f32, vp, i32,
                                  vp, vp, vp, vp, i32, vp, vp, vp, i64, i64, f32, vp, vp, vp, vp, vp, vp, vp]),
    'gga_dcn_im2col': (i32, [vp, vp, vp] + [i32] * 12 + [vp, vp]),
    'gga_dcn_im2col_amax': (i32, [vp, vp, vp] + [i32] * 12 + [vp, vp, vp]),
    'gga_dcn_col2im': (i32, [vp, vp, vp, vp] + [i32] * 12 + [vp, vp, vp, vp]),
    'gga_furthest_point_sample': (i32, [vp, i32, i32, i32, i32, vp, vp, vp]),
    'gga_ball_query': (i32, [vp, vp, i32, i32, i32, f32, f32, i32, vp, vp]),
    'gga_group_points_fwd': (i32, [vp, vp, i32, i32, i32, i64, vp, vp]),
    'gga_group_points_bwd': (i32, [vp, vp, i32, i32, i32, i64, vp, vp]),
    'gga_three_nn': (i32, [vp, vp, i32, i32, i32, vp, vp, vp]),
    'gga_three_interpolate_fwd': (i32, [vp, vp, vp, i32, i32, i32, i32, vp, vp]),
    'gga_three_interpolate_bwd': (i32, [vp, vp, vp, i32, i32, i32, i32, vp, vp]),
    'gga_query_and_group': (i32, [vp, vp, vp, i32, i32, i32, i32, f32, f32, i32, i32, i32, i32, vp, vp, vp]),
    'gga_query_and_group_bwd': (i32, [vp, vp, i32, i32, i32, i32, f32, i32, i32, i32, vp, vp, vp, vp]),
    'gga_group_max_fwd': (i32, [vp, i32, i32, i32, i32, i64, i64, i64, i64, vp, vp, vp]),
    'gga_group_max_bwd': (i32, [vp, vp, i32, i32, i32, i32, i64, i64, i64, i64, vp, vp]),
}


TIME_SCATTER_FWD, TIME_DENSE_CONV, TIME_SPARSE_CONV, TIME_SPARSE_WGRAD, TIME_DENSE_WGRAD = range(5)


def timing_conv_key(cin, cout, hw=0):
    """GGA_TIMING_CONV_KEY of include/gga_hip.h."""
    return (int(cin) << 48) | (int(cout) << 32) | (int(hw) & 0xffffffff)


def timing_begin(site, max_samples, key=0):
    check(lib().gga_timing_begin(site, int(max_samples), int(key)), 'gga_timing_begin')


def timing_collect(site, cap):
    """-> list of per-call milliseconds of the armed session of `site` (waits for its events)."""
    buf = (C.c_float * max(int(cap), 1))()
    n = lib().gga_timing_collect(site, buf, int(cap))
    check(min(n, 0), 'gga_timing_collect')
    return [buf[i] for i in range(n)]


def build(force=False):
    """Compile the HIP sources for gfx950 (hipcc cross-compiles without a GPU)."""
    args = ['make', '-C', os.path.join(_HERE, 'csrc'), '-j4']
    if force:
        args.append('-B')
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f'{LIB_PATH} not found: the GGA HIP kernels are not built. Run '
                '`python -c "import __graft_entry__ as g; g.build()"` (or `make -C gga_amd/csrc`). '
                'There is no CPU fallback for the product path.')
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)       # AttributeError if the .so lacks a declared symbol
            fn.restype, fn.argtypes = res, args
        if L.gga_abi_version() != ABI_VERSION:
            raise RuntimeError(f'libgga_hip.so ABI {L.gga_abi_version()} != binding ABI {ABI_VERSION}; rebuild')
        _lib = L
    return _lib


def check(status, what):
    if status != 0:
        raise RuntimeError(f'{what} failed (status {status}): {lib().gga_last_error().decode()}')
