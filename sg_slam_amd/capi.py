"""ctypes binding of the C-ABI declared in include/sgx.h (one Python method per entry point)."""
import ctypes as C
import numpy as np

KP_DTYPE = np.dtype([('x', 'f4'), ('y', 'f4'), ('size', 'f4'), ('angle', 'f4'), ('response', 'f4'),
                     ('octave', 'i4'), ('class_id', 'i4')])   # cv::KeyPoint / sgx_keypoint, 28 B


class SgxError(RuntimeError):
    pass


class Camera(C.Structure):
    _fields_ = [('fx', C.c_float), ('fy', C.c_float), ('cx', C.c_float), ('cy', C.c_float), ('bf', C.c_float),
                ('min_x', C.c_float), ('max_x', C.c_float), ('min_y', C.c_float), ('max_y', C.c_float)]


class BaProblem(C.Structure):
    _fields_ = [('n_poses', C.c_int32), ('n_points', C.c_int32), ('n_edges', C.c_int32), ('poses', C.c_void_p), ('pose_fixed', C.c_void_p),
                ('points', C.c_void_p), ('edge_pose', C.c_void_p), ('edge_point', C.c_void_p), ('edge_obs', C.c_void_p), ('edge_info', C.c_void_p)]


class BaStats(C.Structure):
    _fields_ = [('iterations_first', C.c_int32), ('iterations_second', C.c_int32), ('free_poses', C.c_int32), ('reserved', C.c_int32),
                ('chi2_first', C.c_double), ('chi2_second', C.c_double)]


SGX_DET_MAX = 100


class Detection(C.Structure):
    _fields_ = [(k, C.c_float) for k in ('label', 'score', 'xmin', 'ymin', 'xmax', 'ymax')]


class Object2D(C.Structure):
    _fields_ = [('id', C.c_int32)] + [(k, C.c_float) for k in ('prob', 'x', 'y', 'w', 'h')]


class DetResult(C.Structure):
    _fields_ = [('n_raw', C.c_int32), ('raw', Detection * SGX_DET_MAX), ('n_objects', C.c_int32), ('objects', Object2D * SGX_DET_MAX),
                ('have_dynamic_for_mapping', C.c_int32), ('have_dynamic_for_rm_feature', C.c_int32),
                ('n_map_boxes', C.c_int32), ('map_boxes', Object2D * SGX_DET_MAX), ('n_rm_boxes', C.c_int32), ('rm_boxes', Object2D * SGX_DET_MAX)]


class FlowConfig(C.Structure):
    _fields_ = [('width', C.c_int32), ('height', C.c_int32), ('max_batch', C.c_int32), ('win_size', C.c_int32), ('max_level', C.c_int32),
                ('max_count', C.c_int32), ('epsilon', C.c_double)]


class TrackerConfig(C.Structure):
    _fields_ = [('streams', C.c_int32), ('width', C.c_int32), ('height', C.c_int32), ('nfeatures', C.c_int32), ('scale_factor', C.c_float), ('nlevels', C.c_int32),
                ('ini_th_fast', C.c_int32), ('min_th_fast', C.c_int32), ('cam', Camera), ('depth_map_factor', C.c_float), ('th_projection', C.c_float),
                ('local_map', C.c_int32), ('dynamic_mask', C.c_int32), ('max_boxes', C.c_int32), ('pipelined', C.c_int32)]


class Obj3dParams(C.Structure):
    _fields_ = [('sor_stddev_mul', C.c_double), ('sor_mean_k', C.c_int32), ('cluster_min_size', C.c_int32), ('cluster_max_size', C.c_int32),
                ('voxel_leaf_size', C.c_float), ('cluster_tolerance', C.c_float), ('similar_compare_ratio', C.c_float),
                ('camera_valid_depth_min', C.c_float), ('camera_valid_depth_max', C.c_float)]


class Obj3dJob(C.Structure):
    _fields_ = [('image', C.c_int32), ('class_id', C.c_int32)] + [(k, C.c_float) for k in ('prob', 'x', 'y', 'w', 'h')]


OBJ3D_RESULT_DTYPE = np.dtype([('found', 'i4'), ('class_id', 'i4'), ('prob', 'f4'), ('centroid', 'f4', 3), ('size', 'f4', 3), ('crop_points', 'i4'), ('kept_points', 'i4'),
                               ('components', 'i4'), ('clusters', 'i4'), ('best_cluster_size', 'i4'), ('larger_window_points', 'i4'), ('best_similar1', 'f4'),
                               ('best_similar2', 'f4'), ('best_roi', 'f4', 4)])   # sgx_obj3d_result, 84 B


class SemanticObjectRecord(C.Structure):
    _fields_ = [('class_id', C.c_int32), ('object_id', C.c_int32), ('prob', C.c_float), ('centroid', C.c_float * 3), ('size', C.c_float * 3)]


class CloudParams(C.Structure):
    _fields_ = [('sor_stddev_mul', C.c_double), ('sor_mean_k', C.c_int32), ('consider_dynamic', C.c_int32), ('voxel_leaf_size', C.c_float),
                ('camera_valid_depth_min', C.c_float), ('camera_valid_depth_max', C.c_float), ('reserved', C.c_int32)]


CLOUD_POINT_DTYPE = np.dtype([('x', 'f4'), ('y', 'f4'), ('z', 'f4'), ('rgba', 'u4')])   # sgx_cloud_point, 16 B: PCL's PointXYZRGB packing
CLOUD_RESULT_DTYPE = np.dtype([('n_points', 'i4'), ('n_pixels_used', 'i4'), ('n_voxels', 'i4'), ('flags', 'i4'), ('larger_window_points', 'i4'), ('reserved', 'i4'),
                               ('mean', 'f8'), ('thr', 'f8')])   # sgx_cloud_result, 40 B
SGX_CLOUD_LOCAL, SGX_CLOUD_WORLD = 0, 1
SGX_CLOUD_FEW_POINTS, SGX_CLOUD_LEAF_TOO_SMALL = 1, 2
SGX_CLOUD_MAX_BOXES = 128


class OctomapParams(C.Structure):
    _fields_ = [(k, C.c_double) for k in ('res', 'prob_hit', 'prob_miss', 'thres_min', 'thres_max', 'max_range', 'pointcloud_min_x', 'pointcloud_max_x', 'pointcloud_min_y',
                                          'pointcloud_max_y', 'pointcloud_min_z', 'pointcloud_max_z', 'occupancy_min_z', 'occupancy_max_z', 'min_size_x', 'min_size_y')]


class OctomapGridHeader(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ('width', 'height', 'flags', 'reserved')] + [('pad_min_key', C.c_int32 * 2), ('pad_max_key', C.c_int32 * 2), ('key_min_z', C.c_int32),
                                                                                     ('key_max_z', C.c_int32)] + [(k, C.c_double) for k in ('resolution', 'origin_x', 'origin_y')]


OCTOMAP_RECORD_DTYPE = np.dtype([(k, 'i4') for k in ('n_in', 'n_passed', 'n_truncated', 'n_bad_end_key', 'n_invalid_rays', 'n_free_updates', 'n_occupied_updates',
                                                     'n_new_cells')] + [('bbx_min', 'i4', 3), ('bbx_max', 'i4', 3), ('flags', 'i4'), ('reserved', 'i4')])   # sgx_octomap_record, 64 B
OCTOMAP_CELL_DTYPE = np.dtype([('key', 'u2', 3), ('reserved', 'u2'), ('x', 'f4'), ('y', 'f4'), ('z', 'f4'), ('logodds', 'f4')])   # sgx_octomap_cell, 24 B
OCTOMAP_BOUNDS_DTYPE = np.dtype([('n_known', 'i4'), ('n_occupied', 'i4'), ('n_free', 'i4'), ('n_bricks', 'i4'), ('key_min', 'i4', 3), ('key_max', 'i4', 3)])   # sgx_octomap_bounds_t, 40 B
SGX_OCTOMAP_ORIGIN_OUT_OF_RANGE, SGX_OCTOMAP_RAY_LEFT_KEYSPACE, SGX_OCTOMAP_MAP_FULL, SGX_OCTOMAP_TOO_MANY_POINTS = 1, 2, 4, 8
SGX_OCTOMAP_GRID_EMPTY, SGX_OCTOMAP_GRID_KEY_OUT_OF_RANGE = 1, 2


class GlobalMapParams(C.Structure):
    _fields_ = [('sor_stddev_mul', C.c_double), ('sor_mean_k', C.c_int32), ('voxel_leaf_size', C.c_float)]


GMAP_APPEND_DTYPE = np.dtype([('n_in', 'i4'), ('offset', 'i4'), ('map_size', 'i4'), ('flags', 'i4')])   # sgx_globalmap_append_record, 16 B
GMAP_RESULT_DTYPE = np.dtype([('n_points_in', 'i4'), ('n_voxels', 'i4'), ('n_points', 'i4'), ('flags', 'i4'), ('wider_window_points', 'i4'), ('whole_cloud_points', 'i4'),
                              ('mean', 'f8'), ('thr', 'f8')])   # sgx_globalmap_result, 40 B
SGX_GMAP_FEW_POINTS, SGX_GMAP_LEAF_TOO_SMALL, SGX_GMAP_FULL = 1, 2, 4
SGX_GMAP_MAX_POINTS, SGX_GMAP_MAX_RADIUS = 1 << 22, 16


class InitReport(C.Structure):
    _fields_ = [('SH', C.c_float), ('SF', C.c_float), ('RH', C.c_float), ('model', C.c_int32), ('n_matches', C.c_int32), ('n_inliers_h', C.c_int32),
                ('n_inliers_f', C.c_int32), ('n_hyp', C.c_int32), ('best_hyp', C.c_int32), ('n_good', C.c_int32 * 8), ('cos_parallax', C.c_float * 8),
                ('parallax', C.c_float * 8), ('H21', C.c_float * 9), ('F21', C.c_float * 9)]


class KfdbReport(C.Structure):
    _fields_ = [('n_sharing', C.c_int32), ('max_common_words', C.c_int32), ('min_common_words', C.c_int32), ('n_scores', C.c_int32), ('n_score_and_match', C.c_int32),
                ('best_acc_score', C.c_float), ('min_score_to_retain', C.c_float), ('n_candidates', C.c_int32), ('status', C.c_int32)]


KFDB_REPORT_DTYPE = np.dtype([('n_sharing', 'i4'), ('max_common_words', 'i4'), ('min_common_words', 'i4'), ('n_scores', 'i4'), ('n_score_and_match', 'i4'),
                              ('best_acc_score', 'f4'), ('min_score_to_retain', 'f4'), ('n_candidates', 'i4'), ('status', 'i4')])   # sgx_kfdb_report, 36 B


COVIS_REPORT_DTYPE = np.dtype([(k, 'i4') for k in ('status', 'n_counter', 'max_weight', 'max_kf', 'n_ordered', 'parent', 'n_stage1', 'n_local_kf', 'n_local_points',
                                                   'ref_tracked')])   # sgx_covis_report, 40 B
COVIS_BA_REPORT_DTYPE = np.dtype([(k, 'i4') for k in ('status', 'n_local_kf', 'n_fixed_kf', 'n_poses', 'n_points', 'n_edges', 'n_mono_edges',
                                                      'n_stereo_edges')])   # sgx_covis_ba_report, 32 B
COVIS_LOOP_REPORT_DTYPE = np.dtype([(k, 'i4') for k in ('status', 'n_group', 'n_points', 'n_connections', 'n_vertices', 'n_edges')] + [('n_kind', 'i4', (4,))])   # sgx_covis_loop_report, 40 B
COVIS_CONSISTENCY_REPORT_DTYPE = np.dtype([(k, 'i4') for k in ('status', 'n_before', 'n_after', 'n_consistent', 'n_pushed_zero', 'n_pushed_nothing', 'n_enough',
                                                               'n_cand')])   # sgx_covis_consistency_report, 32 B
NEWPOINTS_REPORT_DTYPE = np.dtype([('status', 'i4'), ('kf2', 'i4'), ('n_pairs', 'i4'), ('n_new', 'i4'), ('baseline', 'f4'), ('F12', 'f4', (9,)), ('Ow1', 'f4', (3,)),
                                   ('Ow2', 'f4', (3,))])   # sgx_newpoints_report, 80 B
SGX_NEWPOINTS_PROCESSED, SGX_NEWPOINTS_SKIPPED = 0, 1
COVIS_GBA_REPORT_DTYPE = np.dtype([(k, 'i4') for k in ('status', 'n_visited', 'n_propagated', 'n_unreached', 'max_depth')] + [('pad', 'i4', (3,))])   # sgx_covis_gba_report, 32 B


class OrbConfig(C.Structure):
    _fields_ = [('nfeatures', C.c_int32), ('scale_factor', C.c_float), ('nlevels', C.c_int32),
                ('ini_th_fast', C.c_int32), ('min_th_fast', C.c_int32), ('width', C.c_int32),
                ('height', C.c_int32), ('max_batch', C.c_int32)]


# every symbol include/sgx.h declares (tests/test_abi.py checks the export table against this list)
SYMBOLS = [
    'sgx_version', 'sgx_status_string', 'sgx_orb_create', 'sgx_orb_destroy', 'sgx_orb_keypoint_capacity', 'sgx_orb_get_tables',
    'sgx_orb_extract_batch_dev', 'sgx_orb_extract', 'sgx_orb_last_status', 'sgx_profile_enable', 'sgx_profile_num_classes', 'sgx_profile_class_name',
    'sgx_profile_read', 'sgx_match_project_frame_batch_dev', 'sgx_match_project_frame', 'sgx_match_project_local_batch_dev',
    'sgx_match_project_local', 'sgx_frame_stereo_from_rgbd_batch_dev', 'sgx_frame_unproject_batch_dev', 'sgx_frame_make_map_points_batch_dev',
    'sgx_frame_merge_matches_batch_dev', 'sgx_pose_optimization_batch_dev', 'sgx_pose_optimization', 'sgx_frame_motion_model_batch_dev',
    'sgx_local_bundle_adjustment', 'sgx_bundle_adjustment', 'sgx_det_create', 'sgx_det_destroy', 'sgx_det_info', 'sgx_det_detect',
    'sgx_det_detect_batch_dev', 'sgx_det_forward_batch_dev', 'sgx_frame_compact_keys_batch_dev', 'sgx_frame_gray_from_color_batch_dev',
    'sgx_det_gemm_mode', 'sgx_det_plan_step', 'sgx_dynamic_mask_batch_dev', 'sgx_tracker_create', 'sgx_tracker_destroy',
    'sgx_tracker_keypoint_capacity', 'sgx_tracker_record_bytes', 'sgx_tracker_set_initial_pose', 'sgx_tracker_step_dev', 'sgx_tracker_host_buffers',
    'sgx_tracker_step_host', 'sgx_tracker_wait_inputs', 'sgx_tracker_sync', 'sgx_tracker_read', 'sgx_tracker_snapshot_pose_dev',
    'sgx_tracker_snapshot_boxes_dev', 'sgx_tracker_pack_records_dev', 'sgx_tracker_frame_dev', 'sgx_tracker_extractor', 'sgx_flow_create',
    'sgx_dist_unique_id', 'sgx_dist_create', 'sgx_dist_destroy', 'sgx_dist_world', 'sgx_dist_gather_records',
    'sgx_flow_destroy', 'sgx_flow_reset', 'sgx_flow_levels', 'sgx_flow_lk_batch_dev', 'sgx_flow_lk', 'sgx_fundamental_ransac_batch_dev',
    'sgx_find_fundamental_mat', 'sgx_hamming_matrix', 'sgx_hamming_matrix_dev', 'sgx_match_search_for_triangulation', 'sgx_match_search_by_bow',
    'sgx_match_search_by_bow_kf', 'sgx_match_fuse_search', 'sgx_match_project_keyframe', 'sgx_match_fuse_search_sim3',
    'sgx_triangulate_new_map_points', 'sgx_mappoint_update_normal_and_depth', 'sgx_mappoint_distinctive_descriptors', 'sgx_sim3_solver_create',
    'sgx_sim3_solver_set_ransac_parameters', 'sgx_sim3_solver_iterate', 'sgx_sim3_solver_get_estimate', 'sgx_sim3_solver_destroy',
    'sgx_match_search_for_initialization', 'sgx_voc_load', 'sgx_voc_create', 'sgx_voc_info', 'sgx_voc_destroy', 'sgx_voc_transform',
    'sgx_voc_transform_batch_dev', 'sgx_voc_score', 'sgx_match_project_sim3', 'sgx_match_search_by_sim3', 'sgx_optimize_sim3',
    'sgx_optimize_essential_graph', 'sgx_correct_map_points', 'sgx_undistort_points', 'sgx_frame_undistort_stereo_rgbd_batch_dev', 'sgx_frame_image_bounds',
    'sgx_tracker_set_distortion', 'sgx_tracker_frame_keys_un_dev', 'sgx_pnp_solver_create', 'sgx_pnp_solver_set_ransac_parameters', 'sgx_pnp_solver_iterate',
    'sgx_pnp_solver_get_estimate', 'sgx_pnp_solver_destroy', 'sgx_pnp_batch_create', 'sgx_pnp_batch_set_dev', 'sgx_pnp_batch_iterate_dev', 'sgx_pnp_batch_destroy',
    'sgx_obj3d_create', 'sgx_obj3d_destroy', 'sgx_obj3d_detect_batch_dev', 'sgx_obj3d_detect', 'sgx_objdb_create', 'sgx_objdb_destroy', 'sgx_objdb_add', 'sgx_objdb_size',
    'sgx_objdb_get', 'sgx_initializer_create', 'sgx_initializer_initialize', 'sgx_initializer_destroy', 'sgx_init_batch_create', 'sgx_init_batch_run_dev',
    'sgx_init_batch_destroy', 'sgx_orb_detect_batch_dev', 'sgx_orb_describe_batch_dev', 'sgx_frame_compact_keys_src_batch_dev',
    'sgx_voc_bow_batch_dev', 'sgx_kfdb_create', 'sgx_kfdb_destroy', 'sgx_kfdb_size', 'sgx_kfdb_add', 'sgx_kfdb_erase', 'sgx_kfdb_clear', 'sgx_kfdb_set_covisibility',
    'sgx_kfdb_slots', 'sgx_kfdb_detect_relocalization_candidates', 'sgx_kfdb_detect_loop_candidates', 'sgx_kfdb_min_score', 'sgx_kfdb_detect_batch_dev',
    'sgx_cloud_create', 'sgx_cloud_destroy', 'sgx_cloud_build_batch_dev', 'sgx_cloud_build', 'sgx_cloud_camera_to_map_tf',
    'sgx_stereo_create', 'sgx_stereo_destroy', 'sgx_stereo_match_batch_dev', 'sgx_stereo_match',
    'sgx_covis_create', 'sgx_covis_destroy', 'sgx_covis_size', 'sgx_covis_info', 'sgx_covis_clear', 'sgx_covis_add_keyframe', 'sgx_covis_set_observations',
    'sgx_covis_set_points_bad', 'sgx_covis_replace_point', 'sgx_covis_erase_keyframe', 'sgx_covis_get_weights', 'sgx_covis_get_ordered', 'sgx_covis_best_covisibles',
    'sgx_covis_get_tree', 'sgx_covis_get_observations', 'sgx_covis_get_keyframe_points', 'sgx_covis_update_connections_batch_dev', 'sgx_covis_local_map_batch_dev',
    'sgx_covis_keyframe_culling_batch_dev', 'sgx_covis_update_connections', 'sgx_covis_local_map', 'sgx_covis_keyframe_culling', 'sgx_covis_ba_graph_batch_dev',
    'sgx_covis_ba_graph', 'sgx_covis_add_loop_edge', 'sgx_covis_get_loop_edges', 'sgx_covis_loop_info', 'sgx_covis_loop_begin_dev', 'sgx_covis_loop_connections_dev',
    'sgx_covis_essential_graph_dev', 'sgx_covis_loop_begin', 'sgx_covis_loop_connections', 'sgx_covis_essential_graph',
    'sgx_covis_consistency_reserve', 'sgx_covis_consistency_clear', 'sgx_covis_consistency_info', 'sgx_covis_get_consistent_groups', 'sgx_covis_consistency_dev',
    'sgx_covis_connected_batch_dev', 'sgx_covis_consistency', 'sgx_covis_connected_batch', 'sgx_covis_gba_update_dev', 'sgx_gba_correct_points_dev', 'sgx_covis_gba_update', 'sgx_gba_correct_points',
    'sgx_loop_propagate_sim3_dev', 'sgx_eg_flatten_dev', 'sgx_eg_recover_dev', 'sgx_correct_map_points_dev', 'sgx_loop_propagate_sim3', 'sgx_eg_flatten', 'sgx_eg_recover',
    'sgx_octomap_create', 'sgx_octomap_destroy', 'sgx_octomap_reset', 'sgx_octomap_insert_batch_dev', 'sgx_octomap_insert', 'sgx_octomap_bounds', 'sgx_octomap_cells_dev',
    'sgx_octomap_cells', 'sgx_octomap_search_dev', 'sgx_octomap_grid_header', 'sgx_octomap_project_dev', 'sgx_octomap_project', 'sgx_octomap_sensor_to_world',
    'sgx_globalmap_create', 'sgx_globalmap_destroy', 'sgx_globalmap_reset', 'sgx_globalmap_append_batch_dev', 'sgx_globalmap_append', 'sgx_globalmap_consolidate_dev',
    'sgx_globalmap_consolidate', 'sgx_globalmap_size', 'sgx_globalmap_read', 'sgx_globalmap_points_dev',
    'sgx_kfstore_create', 'sgx_kfstore_destroy', 'sgx_kfstore_size', 'sgx_kfstore_info', 'sgx_kfstore_clear', 'sgx_kfstore_add', 'sgx_kfstore_set_pose', 'sgx_kfstore_erase',
    'sgx_create_new_map_points_batch_dev', 'sgx_create_new_map_points',
]
# the test / tuning taps include/sgx_debug.h declares: exported by tests/taps/libsgx_taps.so and the emulator (-DSGX_DEBUG_TAPS) only, never by the product library
TAP_SYMBOLS = [
    'sgx_orb_debug_level_geometry', 'sgx_orb_debug_set_unfused_pyramid', 'sgx_orb_debug_read_level', 'sgx_orb_debug_read_candidates',
    'sgx_orb_debug_run_octree', 'sgx_orb_debug_read_plan', 'sgx_pose_opt_debug_set_threads', 'sgx_ba_debug_set_solver', 'sgx_ba_debug_set_jobs', 'sgx_ba_debug_set_init', 'sgx_ba_debug_last_plan', 'sgx_det_debug_read_blob',
    'sgx_det_debug_detection_output', 'sgx_det_debug_continued', 'sgx_debug_flow_affine_batch_dev', 'sgx_det_debug_set_fusion', 'sgx_det_debug_set_legacy_kernels',
    'sgx_det_debug_set_block_fusion', 'sgx_det_debug_set_irb', 'sgx_det_debug_set_gemm', 'sgx_det_debug_time_ops', 'sgx_det_debug_run_step', 'sgx_flow_debug_read_level',
    'sgx_flow_debug_level_size', 'sgx_flow_debug_read_slot', 'sgx_debug_corun_bf16', 'sgx_pnp_debug_betas', 'sgx_obj3d_debug_read',
    'sgx_tracker_debug_set_describe_early', 'sgx_tracker_debug_set_boxes', 'sgx_tracker_debug_sync_trace', 'sgx_tracker_debug_fail_after',
    'sgx_debug_devmem_fail_after', 'sgx_cloud_debug_read', 'sgx_stereo_debug_read', 'sgx_globalmap_debug_read', 'sgx_globalmap_debug_max_radius',
]


def _vp(x):
    """device/host pointer from int, numpy array or anything with data_ptr()"""
    if x is None:
        return None
    if isinstance(x, int):
        return C.c_void_p(x)
    if hasattr(x, 'data_ptr'):
        return C.c_void_p(x.data_ptr())
    return x.ctypes.data_as(C.c_void_p)


class SgxLib:
    def __init__(self, path):
        self.path = path
        self.dll = C.CDLL(path)
        d = self.dll
        d.sgx_version.restype = C.c_char_p
        d.sgx_status_string.restype = C.c_char_p
        d.sgx_status_string.argtypes = [C.c_int]
        d.sgx_orb_create.argtypes = [C.POINTER(OrbConfig), C.POINTER(C.c_void_p)]
        d.sgx_orb_destroy.argtypes = [C.c_void_p]
        d.sgx_orb_destroy.restype = None
        d.sgx_orb_keypoint_capacity.argtypes = [C.c_void_p]
        d.sgx_orb_get_tables.argtypes = [C.c_void_p] + [C.c_void_p] * 5
        d.sgx_orb_extract_batch_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_int, C.c_void_p]
        d.sgx_orb_detect_batch_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        d.sgx_orb_describe_batch_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        d.sgx_orb_extract.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        d.sgx_orb_last_status.argtypes = [C.c_void_p, C.c_void_p]

        d.sgx_profile_enable.argtypes = [C.c_int]
        d.sgx_profile_class_name.restype = C.c_char_p
        d.sgx_profile_class_name.argtypes = [C.c_int]
        d.sgx_profile_read.argtypes = [C.c_void_p, C.c_void_p, C.c_int]

        vp = C.c_void_p
        d.sgx_match_project_frame_batch_dev.argtypes = [C.c_int, C.c_int] + [vp] * 13 + [C.POINTER(Camera), vp, C.c_int, C.c_float, C.c_int, C.c_int, vp, vp, vp]
        d.sgx_match_project_frame.argtypes = [C.c_int] + [vp] * 4 + [C.c_int] + [vp] * 7 + [C.POINTER(Camera), vp, C.c_int, C.c_float, C.c_int, C.c_int, vp, vp]
        d.sgx_frame_stereo_from_rgbd_batch_dev.argtypes = [C.c_int, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_float, C.c_float, vp, vp, vp]
        d.sgx_frame_unproject_batch_dev.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, C.POINTER(Camera), vp, vp, vp]
        d.sgx_pose_optimization_batch_dev.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int, vp, C.c_int, C.POINTER(Camera), vp, vp, vp, vp]
        d.sgx_pose_optimization.argtypes = [C.c_int, vp, vp, vp, vp, vp, C.c_int, C.POINTER(Camera), vp, vp, vp]
        d.sgx_frame_motion_model_batch_dev.argtypes = [C.c_int, vp, vp, vp, vp, vp]
        d.sgx_local_bundle_adjustment.argtypes = [C.POINTER(BaProblem), C.POINTER(Camera), vp, vp, C.POINTER(BaStats)]
        d.sgx_bundle_adjustment.argtypes = [C.POINTER(BaProblem), C.POINTER(Camera), C.c_int, vp, C.c_int, C.POINTER(BaStats)]
        d.sgx_det_create.argtypes = [C.c_char_p, vp, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.POINTER(vp)]
        d.sgx_det_destroy.argtypes = [vp]; d.sgx_det_destroy.restype = None
        d.sgx_det_info.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double)]
        d.sgx_det_detect.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(DetResult)]
        d.sgx_det_detect_batch_dev.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, vp]
        d.sgx_det_forward_batch_dev.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(vp), vp]
        d.sgx_det_gemm_mode.argtypes = [vp]
        d.sgx_tracker_create.argtypes = [C.POINTER(TrackerConfig), vp, C.POINTER(vp)]
        d.sgx_tracker_destroy.argtypes = [vp]; d.sgx_tracker_destroy.restype = None
        d.sgx_tracker_keypoint_capacity.argtypes = [vp]
        d.sgx_tracker_record_bytes.argtypes = [vp]
        d.sgx_tracker_set_initial_pose.argtypes = [vp, vp]
        d.sgx_tracker_step_dev.argtypes = [vp, vp, C.c_int, vp, vp, C.c_int, vp]
        d.sgx_tracker_host_buffers.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_int), C.POINTER(vp)]
        d.sgx_tracker_step_host.argtypes = [vp, C.c_int, C.c_int]
        d.sgx_tracker_sync.argtypes = [vp]
        d.sgx_tracker_wait_inputs.argtypes = [vp, C.c_int]
        d.sgx_tracker_read.argtypes = [vp] * 10
        d.sgx_tracker_snapshot_pose_dev.argtypes = [vp, vp]
        d.sgx_tracker_snapshot_boxes_dev.argtypes = [vp, C.c_int, vp, vp]
        d.sgx_tracker_pack_records_dev.argtypes = [vp, vp, vp]
        d.sgx_dist_unique_id.argtypes = [vp]
        d.sgx_dist_create.argtypes = [vp, C.c_int, C.c_int, C.POINTER(vp)]
        d.sgx_dist_destroy.argtypes = [vp]; d.sgx_dist_destroy.restype = None
        d.sgx_dist_world.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        d.sgx_dist_gather_records.argtypes = [vp, vp, C.c_size_t, vp, C.c_int, vp]
        d.sgx_tracker_frame_dev.argtypes = [vp] + [C.POINTER(vp)] * 6
        d.sgx_tracker_extractor.argtypes = [vp]; d.sgx_tracker_extractor.restype = vp
        d.sgx_det_plan_step.argtypes = [vp, C.c_int, C.c_char_p, C.c_int]
        d.sgx_dynamic_mask_batch_dev.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp]
        d.sgx_frame_gray_from_color_batch_dev.argtypes = [C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp]
        d.sgx_frame_compact_keys_batch_dev.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp]
        d.sgx_frame_compact_keys_src_batch_dev.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp]
        d.sgx_match_project_local.argtypes = [C.c_int] + [vp] * 5 + [C.c_int] + [vp] * 7 + [C.POINTER(Camera), vp, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, vp, vp, vp]
        d.sgx_match_project_local_batch_dev.argtypes = [C.c_int, C.c_int] + [vp] * 6 + [C.c_int] + [vp] * 8 + [C.POINTER(Camera), vp, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, vp, vp, vp, vp]
        d.sgx_undistort_points.argtypes = [C.c_int, vp, vp, vp, C.c_int, vp]
        d.sgx_frame_undistort_stereo_rgbd_batch_dev.argtypes = [C.c_int, C.c_int, vp, vp, vp, C.c_int, C.POINTER(Camera), vp, C.c_int, C.c_int, C.c_float, vp, vp, vp, vp]
        d.sgx_frame_image_bounds.argtypes = [C.c_int, C.c_int, vp, vp, C.c_int, C.POINTER(Camera)]
        d.sgx_tracker_set_distortion.argtypes = [vp, vp, C.c_int, C.POINTER(Camera)]
        d.sgx_tracker_frame_keys_un_dev.argtypes = [vp, C.POINTER(vp)]
        d.sgx_frame_make_map_points_batch_dev.argtypes = [C.c_int, C.c_int, C.c_int] + [vp] * 7 + [C.c_int] + [vp] * 7
        d.sgx_frame_merge_matches_batch_dev.argtypes = [C.c_int, C.c_int] + [vp] * 10
        d.sgx_flow_create.argtypes = [C.POINTER(FlowConfig), C.POINTER(vp)]
        d.sgx_flow_destroy.argtypes = [vp]; d.sgx_flow_destroy.restype = None
        d.sgx_flow_reset.argtypes = [vp]
        d.sgx_flow_levels.argtypes = [vp]
        d.sgx_flow_lk_batch_dev.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, C.POINTER(C.c_int32), vp]
        d.sgx_flow_lk.argtypes = [vp, vp, vp, C.c_int, vp, C.c_int, vp, vp]
        d.sgx_fundamental_ransac_batch_dev.argtypes = [C.c_int, C.c_int] + [vp] * 6 + [C.c_int, C.c_double, C.c_double, vp, vp, vp, vp]
        d.sgx_find_fundamental_mat.argtypes = [vp, vp, C.c_int, C.c_double, C.c_double, vp, vp, vp]
        d.sgx_hamming_matrix.argtypes = [vp, C.c_int, vp, C.c_int, vp]
        d.sgx_optimize_essential_graph.argtypes = [C.c_int, vp, vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, vp, vp]
        d.sgx_correct_map_points.argtypes = [C.c_int, vp, vp, C.c_int, vp, vp, vp]
        d.sgx_optimize_sim3.argtypes = [C.c_int] + [vp] * 9 + [C.c_float, C.c_int, vp, vp, vp]
        d.sgx_match_project_keyframe.argtypes = [C.c_int] + [vp] * 4 + [C.c_int] + [vp] * 6 + [C.POINTER(Camera), vp, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, vp, vp]
        d.sgx_match_search_by_bow.argtypes = [C.c_int] + [vp] * 4 + [C.c_int] + [vp] * 3 + [C.c_float, C.c_int, vp, vp]
        d.sgx_match_fuse_search_sim3.argtypes = [C.c_int, vp, vp, vp, C.c_int] + [vp] * 6 + [vp, vp, C.c_int, C.c_float, C.c_float, vp, vp, vp]
        d.sgx_match_project_sim3.argtypes = [C.c_int, vp, vp, vp, vp, C.c_int] + [vp] * 6 + [vp, vp, C.c_int, C.c_float, C.c_int, vp, vp]
        d.sgx_match_search_by_sim3.argtypes = ([C.c_int] + [vp] * 8) * 2 + [vp, vp, C.c_int, C.c_float, C.c_float, vp, vp, C.c_float, vp, vp]
        d.sgx_match_search_for_initialization.argtypes = [C.c_int, vp, vp, C.c_int, vp, vp, vp, C.c_int, C.c_float, C.c_int, vp, vp, vp]
        d.sgx_sim3_solver_create.argtypes = [C.c_int] + [vp] * 6 + [C.c_int, C.c_uint, vp]
        d.sgx_sim3_solver_set_ransac_parameters.argtypes = [vp, C.c_double, C.c_int, C.c_int]
        d.sgx_sim3_solver_iterate.argtypes = [vp, C.c_int] + [vp] * 7
        d.sgx_sim3_solver_get_estimate.argtypes = [vp] * 5
        d.sgx_sim3_solver_destroy.argtypes = [vp]; d.sgx_sim3_solver_destroy.restype = None
        d.sgx_pnp_solver_create.argtypes = [C.c_int] + [vp] * 4 + [C.c_uint, vp]
        d.sgx_pnp_solver_set_ransac_parameters.argtypes = [vp, C.c_double, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float]
        d.sgx_pnp_solver_iterate.argtypes = [vp, C.c_int] + [vp] * 7
        d.sgx_pnp_solver_get_estimate.argtypes = [vp] * 6
        d.sgx_pnp_solver_destroy.argtypes = [vp]; d.sgx_pnp_solver_destroy.restype = None
        d.sgx_pnp_batch_create.argtypes = [C.c_int, C.c_int, vp]
        d.sgx_pnp_batch_set_dev.argtypes = [vp, C.c_int] + [vp] * 8
        d.sgx_pnp_batch_iterate_dev.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp, vp, vp]
        d.sgx_pnp_batch_destroy.argtypes = [vp]; d.sgx_pnp_batch_destroy.restype = None
        d.sgx_initializer_create.argtypes = [C.c_int, vp, vp, C.c_float, C.c_int, C.c_uint, vp]
        d.sgx_initializer_initialize.argtypes = [vp, C.c_int] + [vp] * 10
        d.sgx_initializer_destroy.argtypes = [vp]; d.sgx_initializer_destroy.restype = None
        d.sgx_init_batch_create.argtypes = [C.c_int] * 4 + [vp]
        d.sgx_init_batch_run_dev.argtypes = [vp, C.c_int] + [vp] * 9 + [C.c_int] + [vp] * 8
        d.sgx_init_batch_destroy.argtypes = [vp]; d.sgx_init_batch_destroy.restype = None
        d.sgx_obj3d_create.argtypes = [C.c_int] * 5 + [C.POINTER(Obj3dParams), C.POINTER(vp)]
        d.sgx_obj3d_destroy.argtypes = [vp]; d.sgx_obj3d_destroy.restype = None
        d.sgx_obj3d_detect_batch_dev.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, vp]
        d.sgx_obj3d_detect.argtypes = [vp, vp, vp, vp, C.POINTER(Obj3dJob), vp]
        d.sgx_objdb_create.argtypes = [C.POINTER(vp)]
        d.sgx_objdb_destroy.argtypes = [vp]; d.sgx_objdb_destroy.restype = None
        d.sgx_objdb_add.argtypes = [vp, C.POINTER(SemanticObjectRecord), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        d.sgx_objdb_size.argtypes = [vp]
        d.sgx_objdb_get.argtypes = [vp, C.c_int, C.POINTER(SemanticObjectRecord)]
        d.sgx_cloud_create.argtypes = [C.c_int] * 5 + [C.POINTER(CloudParams), C.POINTER(vp)]
        d.sgx_cloud_destroy.argtypes = [vp]; d.sgx_cloud_destroy.restype = None
        d.sgx_cloud_build_batch_dev.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.c_int] + [vp] * 8
        d.sgx_cloud_build.argtypes = [vp] * 6 + [C.c_int, C.c_int, vp, C.c_int, vp]
        d.sgx_cloud_camera_to_map_tf.argtypes = [vp, vp, vp]
        d.sgx_stereo_create.argtypes = [vp, C.c_int, C.POINTER(vp)]
        d.sgx_stereo_destroy.argtypes = [vp]; d.sgx_stereo_destroy.restype = None
        d.sgx_stereo_match_batch_dev.argtypes = [vp, C.c_int] + [vp, C.c_int, vp, C.c_int] * 2 + [C.c_int] + [vp] * 6 + [C.c_float, C.c_float, vp, vp, vp, vp]
        d.sgx_stereo_match.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp, vp, C.c_int, C.c_float, C.c_float, vp, vp, vp]
        d.sgx_mappoint_update_normal_and_depth.argtypes = [C.c_int] + [vp] * 6 + [C.c_int, vp, vp, vp]
        d.sgx_mappoint_distinctive_descriptors.argtypes = [C.c_int, vp, vp, vp, vp]
        d.sgx_triangulate_new_map_points.argtypes = [C.c_int, vp] + [C.c_int] + [vp] * 5 + [C.c_int] + [vp] * 5 + [vp, vp, vp, C.c_int, vp, vp, vp]
        d.sgx_voc_load.argtypes = [C.c_char_p, vp]
        d.sgx_voc_create.argtypes = [C.c_int] * 5 + [vp] * 5
        d.sgx_voc_info.argtypes = [vp] * 7
        d.sgx_voc_destroy.argtypes = [vp]; d.sgx_voc_destroy.restype = None
        d.sgx_voc_transform.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp]
        d.sgx_voc_transform_batch_dev.argtypes = [vp, vp, C.c_size_t, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
        d.sgx_voc_score.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, vp, vp]
        d.sgx_voc_bow_batch_dev.argtypes = [vp, vp, C.c_int, C.c_int] + [vp] * 6
        d.sgx_kfdb_create.argtypes = [vp] + [C.c_int] * 4 + [vp]
        d.sgx_kfdb_destroy.argtypes = [vp]; d.sgx_kfdb_destroy.restype = None
        d.sgx_kfdb_size.argtypes = [vp]
        d.sgx_kfdb_add.argtypes = [vp, C.c_int32, C.c_int, vp, vp]
        d.sgx_kfdb_erase.argtypes = [vp, C.c_int32]
        d.sgx_kfdb_clear.argtypes = [vp]
        d.sgx_kfdb_set_covisibility.argtypes = [vp, C.c_int32, C.c_int, vp]
        d.sgx_kfdb_slots.argtypes = [vp, vp, vp]
        d.sgx_kfdb_detect_relocalization_candidates.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.POINTER(KfdbReport)]
        d.sgx_kfdb_detect_loop_candidates.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, C.c_float, vp, vp, C.POINTER(KfdbReport)]
        d.sgx_kfdb_min_score.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, vp]
        d.sgx_kfdb_detect_batch_dev.argtypes = [vp, C.c_int, C.c_int, vp, vp, C.c_int] + [vp] * 10
        d.sgx_covis_create.argtypes = [C.c_int] * 6 + [C.c_float, vp]
        d.sgx_covis_destroy.argtypes = [vp]; d.sgx_covis_destroy.restype = None
        d.sgx_covis_size.argtypes = [vp]
        d.sgx_covis_info.argtypes = [vp, vp, vp, vp]
        d.sgx_covis_clear.argtypes = [vp]
        d.sgx_covis_add_keyframe.argtypes = [vp, C.c_int32, C.c_int, vp, vp, vp]
        d.sgx_covis_set_observations.argtypes = [vp, C.c_int32, C.c_int, vp, vp]
        d.sgx_covis_set_points_bad.argtypes = [vp, C.c_int, vp]
        d.sgx_covis_replace_point.argtypes = [vp, C.c_int32, C.c_int32]
        d.sgx_covis_erase_keyframe.argtypes = [vp, C.c_int32]
        d.sgx_covis_get_weights.argtypes = [vp, C.c_int32, vp, vp, vp]
        d.sgx_covis_get_ordered.argtypes = [vp, C.c_int32, vp, vp, vp]
        d.sgx_covis_best_covisibles.argtypes = [vp, C.c_int32, C.c_int, vp, vp]
        d.sgx_covis_get_tree.argtypes = [vp, C.c_int32, vp, vp, vp, vp]
        d.sgx_covis_get_observations.argtypes = [vp, C.c_int32, vp, vp, vp, vp]
        d.sgx_covis_get_keyframe_points.argtypes = [vp, C.c_int32, vp, vp]
        d.sgx_covis_update_connections_batch_dev.argtypes = [vp, C.c_int, vp, vp, vp]
        d.sgx_covis_local_map_batch_dev.argtypes = [vp, C.c_int, C.c_int] + [vp] * 7 + [C.c_int] + [vp] * 5
        d.sgx_covis_keyframe_culling_batch_dev.argtypes = [vp, C.c_int, vp, C.c_int] + [vp] * 6
        d.sgx_covis_update_connections.argtypes = [vp, C.c_int32, vp]
        d.sgx_covis_local_map.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp]
        d.sgx_covis_keyframe_culling.argtypes = [vp, C.c_int32, C.c_int, vp, vp, vp, vp, vp]
        d.sgx_covis_ba_graph_batch_dev.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, vp, C.c_int] + [vp] * 6
        d.sgx_covis_ba_graph.argtypes = [vp, C.c_int, C.c_int32, vp, vp, C.c_int, vp, vp, C.c_int] + [vp] * 5
        d.sgx_covis_add_loop_edge.argtypes = [vp, C.c_int32, C.c_int32]
        d.sgx_covis_get_loop_edges.argtypes = [vp, C.c_int32, vp, vp]
        d.sgx_covis_loop_info.argtypes = [vp, vp, vp]
        d.sgx_covis_loop_begin_dev.argtypes = [vp, C.c_int32, vp, vp, C.c_int, vp, vp, vp, vp]
        d.sgx_covis_loop_connections_dev.argtypes = [vp, C.c_int32, C.c_int, vp, C.c_int, vp, vp, vp, vp]
        d.sgx_covis_essential_graph_dev.argtypes = [vp, C.c_int32, C.c_int32, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp]
        d.sgx_covis_loop_begin.argtypes = [vp, C.c_int32, vp, vp, C.c_int, vp, vp, vp]
        d.sgx_covis_loop_connections.argtypes = [vp, C.c_int32, C.c_int, vp, C.c_int, vp, vp, vp]
        d.sgx_covis_essential_graph.argtypes = [vp, C.c_int32, C.c_int32, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp]
        d.sgx_covis_consistency_reserve.argtypes = [vp, C.c_int]
        d.sgx_covis_consistency_clear.argtypes = [vp]
        d.sgx_covis_consistency_info.argtypes = [vp, vp, vp, vp]
        d.sgx_covis_get_consistent_groups.argtypes = [vp, vp, vp, vp, C.c_int, vp]
        d.sgx_covis_consistency_dev.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp, vp]
        d.sgx_covis_connected_batch_dev.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, vp, vp]
        d.sgx_covis_consistency.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp, vp]
        d.sgx_covis_connected_batch.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, vp]
        d.sgx_covis_gba_update_dev.argtypes = [vp, C.c_int, vp, C.c_int] + [vp] * 9
        d.sgx_gba_correct_points_dev.argtypes = [C.c_int] + [vp] * 9
        d.sgx_covis_gba_update.argtypes = [vp, C.c_int, vp, C.c_int] + [vp] * 8
        d.sgx_gba_correct_points.argtypes = [C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp]
        d.sgx_loop_propagate_sim3_dev.argtypes = [C.c_int, vp, vp, vp, vp, vp, vp]
        d.sgx_eg_flatten_dev.argtypes = [C.c_int, vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]
        d.sgx_eg_recover_dev.argtypes = [C.c_int, vp, vp, vp, vp]
        d.sgx_correct_map_points_dev.argtypes = [C.c_int, vp, vp, vp, vp, vp, vp]
        d.sgx_loop_propagate_sim3.argtypes = [C.c_int, vp, vp, vp, vp, vp]
        d.sgx_eg_flatten.argtypes = [C.c_int, vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp, vp]
        d.sgx_eg_recover.argtypes = [C.c_int, vp, vp, vp]
        d.sgx_octomap_create.argtypes = [C.POINTER(OctomapParams), C.c_int, C.c_int, C.POINTER(vp)]
        d.sgx_octomap_destroy.argtypes = [vp]; d.sgx_octomap_destroy.restype = None
        d.sgx_octomap_reset.argtypes = [vp]
        d.sgx_octomap_insert_batch_dev.argtypes = [vp, vp, C.c_int64, vp, C.c_int64, vp, C.c_int, vp, vp]
        d.sgx_octomap_insert.argtypes = [vp, vp, C.c_int, vp, vp]
        d.sgx_octomap_bounds.argtypes = [vp, vp]
        d.sgx_octomap_cells_dev.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp]
        d.sgx_octomap_cells.argtypes = [vp, C.c_int, vp, C.c_int, vp]
        d.sgx_octomap_search_dev.argtypes = [vp, vp, vp, C.c_int, vp, vp]
        d.sgx_octomap_grid_header.argtypes = [vp, vp, C.POINTER(OctomapGridHeader)]
        d.sgx_octomap_project_dev.argtypes = [vp, C.POINTER(OctomapGridHeader), vp, vp]
        d.sgx_octomap_project.argtypes = [vp, C.POINTER(OctomapGridHeader), vp, C.c_int64]
        d.sgx_octomap_sensor_to_world.argtypes = [vp, vp, vp]
        d.sgx_globalmap_create.argtypes = [C.c_int, C.POINTER(GlobalMapParams), C.POINTER(vp)]
        d.sgx_globalmap_destroy.argtypes = [vp]; d.sgx_globalmap_destroy.restype = None
        d.sgx_globalmap_reset.argtypes = [vp]
        d.sgx_globalmap_append_batch_dev.argtypes = [vp, vp, C.c_int64, vp, C.c_int64, C.c_int, vp, vp]
        d.sgx_globalmap_append.argtypes = [vp, vp, C.c_int, vp]
        d.sgx_globalmap_consolidate_dev.argtypes = [vp, vp, vp]
        d.sgx_globalmap_consolidate.argtypes = [vp, vp]
        d.sgx_globalmap_size.argtypes = [vp, vp]
        d.sgx_globalmap_read.argtypes = [vp, vp, C.c_int, vp]
        d.sgx_globalmap_points_dev.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
        d.sgx_kfstore_create.argtypes = [C.c_int, C.c_int, C.POINTER(Camera), vp, vp, C.c_int, vp]
        d.sgx_kfstore_destroy.argtypes = [vp]; d.sgx_kfstore_destroy.restype = None
        d.sgx_kfstore_size.argtypes = [vp]
        d.sgx_kfstore_info.argtypes = [vp, vp, vp]
        d.sgx_kfstore_clear.argtypes = [vp]
        d.sgx_kfstore_add.argtypes = [vp, C.c_int32, C.c_int] + [vp] * 7
        d.sgx_kfstore_set_pose.argtypes = [vp, C.c_int32, vp]
        d.sgx_kfstore_erase.argtypes = [vp, C.c_int32]
        d.sgx_create_new_map_points_batch_dev.argtypes = [vp, C.c_int] + [vp] * 20
        d.sgx_create_new_map_points.argtypes = [vp, C.c_int32, C.c_int, vp, C.c_int32] + [vp] * 15
        d.sgx_match_search_by_bow_kf.argtypes = [C.c_int] + [vp] * 4 + [C.c_int] + [vp] * 4 + [C.c_float, C.c_int, vp, vp]
        d.sgx_match_fuse_search.argtypes = [C.c_int] + [vp] * 4 + [C.c_int] + [vp] * 6 + [C.POINTER(Camera), vp, vp, C.c_int, C.c_float, C.c_float, vp, vp, vp]
        d.sgx_hamming_matrix_dev.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp]
        d.sgx_match_search_for_triangulation.argtypes = [C.c_int] + [vp] * 6 + [C.c_int] + [vp] * 6 + [vp, C.POINTER(Camera), vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]

        # test / tuning taps (include/sgx_debug.h): present in tests/taps/libsgx_taps.so and the emulator only
        self.has_taps = hasattr(d, 'sgx_det_debug_read_blob')
        if self.has_taps:
            d.sgx_orb_debug_level_geometry.argtypes = [C.c_void_p, C.c_int] + [C.POINTER(C.c_int32)] * 3
            d.sgx_orb_debug_read_level.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
            d.sgx_orb_debug_read_candidates.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
            d.sgx_orb_debug_run_octree.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
            d.sgx_orb_debug_set_unfused_pyramid.argtypes = [C.c_int]
            if hasattr(d, 'sgx_orb_debug_read_plan'):      # a tap library built before this entry existed still loads; tap() then reports the missing symbol
                d.sgx_orb_debug_read_plan.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
            d.sgx_pose_opt_debug_set_threads.argtypes = [C.c_int]
            d.sgx_ba_debug_set_solver.argtypes = [C.c_int]
            d.sgx_ba_debug_set_jobs.argtypes = [C.c_int]
            d.sgx_ba_debug_set_init.argtypes = [C.c_int]
            d.sgx_ba_debug_last_plan.argtypes = [C.c_void_p]
            d.sgx_det_debug_detection_output.argtypes = [vp, vp, vp, C.c_int, C.POINTER(DetResult)]
            d.sgx_det_debug_continued.argtypes = [vp, C.POINTER(C.c_int)]
            d.sgx_det_debug_read_blob.argtypes = [vp, C.c_char_p, C.c_int, vp, C.c_int, C.POINTER(C.c_int)]
            for nm in ('fusion', 'legacy_kernels', 'block_fusion', 'irb', 'gemm'):
                getattr(d, 'sgx_det_debug_set_' + nm).argtypes = [C.c_int]
            d.sgx_det_debug_time_ops.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.POINTER(C.c_int)]
            d.sgx_det_debug_run_step.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]
            d.sgx_debug_flow_affine_batch_dev.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_int, vp, vp]
            d.sgx_flow_debug_read_level.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]
            d.sgx_debug_corun_bf16.argtypes = [C.c_int, C.c_int, C.c_int, vp]
            d.sgx_pnp_debug_betas.argtypes = [C.c_int, vp, vp, vp]
            d.sgx_obj3d_debug_read.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.POINTER(C.c_int)]
            d.sgx_flow_debug_level_size.argtypes = [vp, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
            d.sgx_flow_debug_read_slot.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.POINTER(C.c_int32)]
            d.sgx_tracker_debug_set_describe_early.argtypes = [C.c_int]
            d.sgx_tracker_debug_set_boxes.argtypes = [vp, vp, vp, vp]
            if hasattr(d, 'sgx_tracker_debug_sync_trace'):      # as sgx_orb_debug_read_plan: a tap library built before these two existed still loads
                d.sgx_tracker_debug_sync_trace.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_int)]
            if hasattr(d, 'sgx_tracker_debug_fail_after'):
                d.sgx_tracker_debug_fail_after.argtypes = [C.c_int]
            if hasattr(d, 'sgx_debug_devmem_fail_after'):
                d.sgx_debug_devmem_fail_after.argtypes = [C.c_int]
            if hasattr(d, 'sgx_cloud_debug_read'):
                d.sgx_cloud_debug_read.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, C.POINTER(C.c_int)]
            if hasattr(d, 'sgx_stereo_debug_read'):
                d.sgx_stereo_debug_read.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp]
            if hasattr(d, 'sgx_globalmap_debug_read'):
                d.sgx_globalmap_debug_read.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.POINTER(C.c_int)]
                d.sgx_globalmap_debug_max_radius.argtypes = [vp, C.c_int]

    def tap(self, name):
        """a test / tuning tap entry (include/sgx_debug.h); the product library has none"""
        if not self.has_taps:
            raise SgxError(f'{name}: {self.path} is the product build and has no test taps; use tests/taps/libsgx_taps.so (make -C sg_slam_amd/csrc taps)')
        return getattr(self.dll, name)

    def version(self):
        return self.dll.sgx_version().decode()

    def check(self, rc, what=''):
        if rc != 0:
            raise SgxError(f'{what}: {self.dll.sgx_status_string(rc).decode()} ({rc})')

    # per-kernel HIP-event timing (process-wide)
    def profile_enable(self, on=True):
        self.check(self.dll.sgx_profile_enable(int(on)))

    def profile_read(self, reset=True):
        n = self.dll.sgx_profile_num_classes()
        ms = np.zeros(n, 'f4'); cnt = np.zeros(n, 'i4')
        self.check(self.dll.sgx_profile_read(_vp(ms), _vp(cnt), int(reset)), 'sgx_profile_read')
        return {self.dll.sgx_profile_class_name(k).decode(): (float(ms[k]), int(cnt[k])) for k in range(n)}
