"""ctypes binding of the C-ABI in include/travgpu.h (libtravgpu.so).

This is the only way Python (tests, bench.py) reaches the HIP chain.  There is no fallback: if the
shared library is missing this module raises, and without a gfx950 device te_create() fails.
"""
import ctypes as C
import os
import struct
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TRAVGPU_LIB") or os.path.join(_HERE, "libtravgpu.so")

TE_OK = 0
TE_ERR_INVALID_ARG, TE_ERR_BAD_PARAM, TE_ERR_NOT_READY, TE_ERR_HIP, TE_ERR_NO_DEVICE, TE_ERR_UNSUPPORTED = \
    -1, -2, -3, -4, -5, -6

LAYERS = dict(elevation=0, traversability_slope=1, traversability_step=2, traversability_roughness=3,
              traversability=4, traversability_footprint=5, surface_normal_x=6, surface_normal_y=7,
              surface_normal_z=8, slope_footprint=9, step_footprint=10, roughness_footprint=11,
              traversability_x=12, traversability_rot=13, robot_slope=14)
FILTERS = dict(slope=1, step=2, roughness=3, combine=4, normals=5)
RUN_KEEP_NORMALS = 0x1
RUN_FOOTPRINT = 0x2
RUN_GENERIC_KERNELS = 0x4
RUN_FOOTPRINT_MEMO = 0x8
RUN_SEQUENTIAL = 0x10
RUN_NORMALS_ONLY = 0x20
OPT_FP_BLOCKED_WALK, OPT_FP_BLOCKED_BLOCKS_PER_CU, OPT_POLYGON_PER_CELL, OPT_GRAPH_REPLAY, OPT_BCAST_RCCL, OPT_NORMALS_RANK_RULE = 1, 2, 3, 4, 5, 6
OPT_FP_ANY_REACH = 7  # circular footprint: 0 routes by reach (above 20 cells: the route of any reach), 1 that route always
OPT_FACE_FLAGS = 9  # mask kernel of the footprint pass: 1 (default) skips the step-check staging on tiles the upload found without a vertical face, 0 never (identical layers)
OPT_MEDIAN_ROUTE = 10  # te_run_median_fill: 0 by plan, 1 the tile kernel wherever its window fits, 2 the general kernel always (identical layers)
OPT_RADIUS_ROUTE = 11  # te_run_radius_filter: 0 by plan, 1 the sliding kernel wherever its result is provably exact, 2 the in-order gather always (identical layers)
OPT_WINDOW_EXPR_ROUTE = 12  # te_run_window_expression: 0 by plan, 1 the separable route wherever allowed, 2 the direct walk always (identical layers)
EDGE_INSIDE, EDGE_CROP, EDGE_EMPTY, EDGE_MEAN = 0, 1, 2, 3  # te_window_expr_params.edge_handling
EDGE_HANDLING = {"inside": EDGE_INSIDE, "crop": EDGE_CROP, "empty": EDGE_EMPTY, "mean": EDGE_MEAN}
RADIUS_MEAN, RADIUS_MIN = 1, 2  # te_run_radius_filter: gridMapFilters/MeanInRadiusFilter, MinInRadiusFilter
OPT_NORMALS_ALGORITHM = 13  # NormalVectorsFilter: 0 the area method (default), 1 the raster method (finite differences of the four neighbours; changes the layers)
OPT_DISTANCE_ROUTE = 14  # te_run_distance: 0 by plan, 1 the tiled route wherever its tile fits in LDS, 2 the route of any reach always (identical layers)
# te_run_distance: which cells are seeds (NAN_IS_SEED is or-ed in); the two TIME bits are te_time_distance_samples' alone
DISTANCE_BELOW, DISTANCE_ABOVE, DISTANCE_NAN_IS_SEED = 1, 2, 4
DISTANCE_TIME_PASS1, DISTANCE_TIME_PASS2 = 0x100, 0x200
DISTANCE_MODES = {"below": DISTANCE_BELOW, "above": DISTANCE_ABOVE}
# te_run_components / te_run_reachable: the neighbours of a cell, and the most start cells of one call
COMPONENTS_CONNECTIVITY_4, COMPONENTS_CONNECTIVITY_8 = 4, 8
REACHABLE_MAX_STARTS = 256
OPT_FILTER_ANY_RADIUS = 8  # filter discs: 0 up to 32 cells (TE_ERR_UNSUPPORTED above), 1 any radius, 2 the route of any radius for every disc

# every symbol include/travgpu.h declares (tests/test_cabi.py checks the library exports them all)
SYMBOLS = ["te_params_default", "te_params_validate", "te_device_count", "te_create", "te_destroy",
           "te_set_params", "te_get_params", "te_set_option", "te_download_face_flags", "te_set_geometry", "te_upload_elevation", "te_upload_tile", "te_download_tile",
           "te_upload_tile_async", "te_download_tile_async",
           "te_device_ptr", "te_set_layer_present", "te_upload_layer", "te_upload_layer_tile", "te_prefetch_layers", "te_wait_prefetch", "te_upload_layer_circular", "te_download_layer_circular", "te_run_filter", "te_run_chain", "te_run_chain_region", "te_run_footprint", "te_check_footprint_paths", "te_check_footprint_paths_radius",
           "te_sync",
           "te_download_layer", "te_time_chain", "te_time_chain_samples", "te_last_error", "te_version",
           "te_msg_parse", "te_msg_layer", "te_msg_write", "te_upload_msg", "te_download_msg", "te_bag_find_message",
           "te_bag_write", "te_run_polygon_footprint", "te_polygons_traversable",
           "te_check_polygon_footprint_paths", "te_pin_host", "te_unpin_host", "te_path_polygons",
           "te_shard_range", "te_bcast_params", "te_run_chain_multi", "te_sync_multi",
           "te_set_check_robot_inclination", "te_check_inclination", "te_polygon_untraversable_hull",
           "te_image_parse", "te_upload_image", "te_upload_image_msg",
           "te_download_occupancy", "te_download_occupancy_msg", "te_occupancy_msg_write", "te_occupancy_parse",
           "te_download_cloud", "te_download_cloud_msg", "te_cloud_msg_write", "te_cloud_parse", "te_cloud_field", "te_cloud_spans",
           "te_submap_geometry", "te_download_submap", "te_download_submap_msg",
           "te_move_geometry", "te_move_map",
           "te_expr_check", "te_run_expression", "te_run_expression_region", "te_run_chain_region_expression", "te_time_expression_samples",
           "te_median_fill_params_default", "te_median_fill_params_validate", "te_run_median_fill", "te_run_median_fill_region", "te_download_fill_mask",
           "te_time_median_fill_samples",
           "te_run_radius_filter", "te_run_radius_filter_region", "te_radius_filter_stats", "te_time_radius_filter_samples",
           "te_run_distance", "te_run_distance_region", "te_distance_stats", "te_time_distance_samples",
           "te_run_components", "te_run_reachable", "te_components_stats",
           "te_window_expr_params_default", "te_window_expr_params_validate", "te_window_expr_check", "te_run_window_expression", "te_run_window_expression_region",
           "te_window_expression_stats", "te_time_window_expression_samples",
           "te_add_layer", "te_remove_layer", "te_layer_id", "te_layer_name",
           "te_expr_check_ctx", "te_run_layer_expression", "te_run_layer_expression_region",
           "te_run_threshold", "te_run_threshold_region", "te_copy_layer",
           "te_run_layer_expression_thresholds", "te_run_layer_expression_thresholds_region"]
LAYER_COUNT, MAX_USER_LAYERS, MAX_FUSED_THRESHOLDS = 15, 16, 4
THRESHOLD_LOWER, THRESHOLD_UPPER = 1, 2  # te_run_threshold: gridMapFilters/ThresholdFilter lower_threshold / upper_threshold
THRESHOLD_MODES = {"lower": THRESHOLD_LOWER, "upper": THRESHOLD_UPPER}
MSG_MAX_NAME = 64
OCCUPANCY_MAX_LAYERS = CLOUD_MAX_LAYERS = SUBMAP_MAX_LAYERS = 16
POINTFIELD_FLOAT32 = 7


def shard_range(batch, n_shards, k):
    first, count = C.c_int(), C.c_int()
    _check(load().te_shard_range(int(batch), int(n_shards), int(k), C.byref(first), C.byref(count)))
    return first.value, count.value


def _handles(ctxs):
    return (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])


def bcast_params(ctxs, root=0):
    """Every context receives the parameters of ctxs[root] (RCCL across devices, host copy within one)."""
    _check(load().te_bcast_params(_handles(ctxs), len(ctxs), int(root)))


def run_chain_multi(ctxs, flags=0):
    _check(load().te_run_chain_multi(_handles(ctxs), len(ctxs), int(flags)))


def sync_multi(ctxs):
    _check(load().te_sync_multi(_handles(ctxs), len(ctxs)))


def pack_paths(paths):
    """List of (n_i, 2) pose arrays -> (offsets int32[n+1], xy float64[total, 2])."""
    paths = [np.asarray(p, dtype=np.float64).reshape(-1, 2) for p in paths]
    n = len(paths)
    off = np.zeros(n + 1, np.int32)
    if n:
        off[1:] = np.cumsum([len(p) for p in paths])
    xy = np.ascontiguousarray(np.concatenate(paths) if n and off[-1] else np.zeros((1, 2)), dtype=np.float64)
    return off, xy


class TeMsgInfo(C.Structure):
    """te_msg_info: the non-layer part of a grid_map_msgs/GridMap message."""
    _fields_ = [("seq", C.c_uint32), ("stamp_sec", C.c_uint32), ("stamp_nsec", C.c_uint32),
                ("frame_id", C.c_char * MSG_MAX_NAME),
                ("resolution", C.c_double), ("length_x", C.c_double), ("length_y", C.c_double),
                ("pose", C.c_double * 7),
                ("rows", C.c_int32), ("cols", C.c_int32), ("start_row", C.c_int32), ("start_col", C.c_int32),
                ("n_layers", C.c_int32), ("n_basic_layers", C.c_int32)]


class TeImageInfo(C.Structure):
    """te_image_info: a sensor_msgs/Image without its pixels."""
    _fields_ = [("seq", C.c_uint32), ("stamp_sec", C.c_uint32), ("stamp_nsec", C.c_uint32),
                ("frame_id", C.c_char * MSG_MAX_NAME),
                ("height", C.c_int32), ("width", C.c_int32), ("step", C.c_int32),
                ("channels", C.c_int32), ("bytes_per_channel", C.c_int32), ("is_bigendian", C.c_int32),
                ("encoding", C.c_char * MSG_MAX_NAME)]


class TeOccupancyInfo(C.Structure):
    """te_occupancy_info: a nav_msgs/OccupancyGrid without its cells."""
    _fields_ = [("seq", C.c_uint32), ("stamp_sec", C.c_uint32), ("stamp_nsec", C.c_uint32),
                ("frame_id", C.c_char * MSG_MAX_NAME),
                ("map_load_sec", C.c_uint32), ("map_load_nsec", C.c_uint32),
                ("resolution", C.c_float), ("width", C.c_uint32), ("height", C.c_uint32),
                ("origin", C.c_double * 7)]


class TeCloudInfo(C.Structure):
    """te_cloud_info: a sensor_msgs/PointCloud2 without its fields and points."""
    _fields_ = [("seq", C.c_uint32), ("stamp_sec", C.c_uint32), ("stamp_nsec", C.c_uint32),
                ("frame_id", C.c_char * MSG_MAX_NAME),
                ("height", C.c_uint32), ("width", C.c_uint32),
                ("n_fields", C.c_uint32), ("point_step", C.c_uint32), ("row_step", C.c_uint32),
                ("is_bigendian", C.c_int32), ("is_dense", C.c_int32)]


class TeSubmapInfo(C.Structure):
    """te_submap_info: what GridMap::getSubmap makes of a request -- the rectangle in the map and the submap's own geometry."""
    _fields_ = [("ok", C.c_int32), ("row0", C.c_int32), ("col0", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32),
                ("pos_x", C.c_double), ("pos_y", C.c_double), ("length_x", C.c_double), ("length_y", C.c_double)]


class TeMoveInfo(C.Structure):
    """te_move_info: the plan of one move -- the shift in cells, the position held afterwards, the rectangles to refresh
    (row0, col0, h, w; rect_exposed 1: upload its cells first, 0: a trailing line, re-filter only) and whether the results
    computed at the old position were kept."""
    _fields_ = [("shift_rows", C.c_int32), ("shift_cols", C.c_int32), ("n_rects", C.c_int32), ("results_kept", C.c_int32),
                ("all_exposed", C.c_int32), ("_pad0", C.c_int32), ("pos_x", C.c_double), ("pos_y", C.c_double),
                ("rects", (C.c_int32 * 4) * 4), ("rect_exposed", C.c_int32 * 4)]

    def rectangles(self):
        """[((row0, col0, h, w), exposed)] in the plan's order."""
        return [(tuple(int(v) for v in self.rects[k]), bool(self.rect_exposed[k])) for k in range(self.n_rects)]


# encoding name -> (channels, bytes per channel): the encodings te_image_parse accepts
IMAGE_ENCODINGS = {"mono8": (1, 1), "8UC1": (1, 1), "mono16": (1, 2), "16UC1": (1, 2),
                   "rgb8": (3, 1), "bgr8": (3, 1), "8UC3": (3, 1), "rgba8": (4, 1), "bgra8": (4, 1), "8UC4": (4, 1),
                   "rgb16": (3, 2), "bgr16": (3, 2), "16UC3": (3, 2), "rgba16": (4, 2), "bgra16": (4, 2), "16UC4": (4, 2)}


class TeExprInfo(C.Structure):
    _fields_ = [("n_instructions", C.c_int32), ("layer_mask", C.c_uint32), ("n_reductions", C.c_int32), ("stack_depth", C.c_int32)]


class TeThreshold(C.Structure):
    _fields_ = [("mode", C.c_int32), ("_pad", C.c_int32), ("threshold", C.c_double), ("set_to", C.c_double)]


class TeMedianFillParams(C.Structure):
    """te_median_fill_params: the settings of a gridMapFilters/MedianFillFilter entry."""
    _fields_ = [("size", C.c_uint32), ("abi_version", C.c_uint32), ("fill_hole_radius", C.c_double),
                ("filter_existing_values", C.c_int32), ("_pad0", C.c_int32), ("existing_value_radius", C.c_double),
                ("num_erode_dilation_iterations", C.c_int32), ("_pad1", C.c_int32)]


class TeWindowExprParams(C.Structure):
    """te_window_expr_params: the settings of a gridMapFilters/SlidingWindowMathExpressionFilter entry."""
    _fields_ = [("size", C.c_uint32), ("abi_version", C.c_uint32), ("window_size", C.c_int32), ("use_window_length", C.c_int32),
                ("window_length", C.c_double), ("compute_empty_cells", C.c_int32), ("edge_handling", C.c_int32)]


class TePathCheckStats(C.Structure):
    """te_path_check_stats: centres visited, distinct (cell, radius) discs evaluated, distinct radii."""
    _fields_ = [("n_visits", C.c_int), ("n_discs", C.c_int), ("n_radius_classes", C.c_int)]


class TeParams(C.Structure):
    _fields_ = [("size", C.c_uint32), ("abi_version", C.c_uint32),
                ("normals_radius", C.c_double), ("normals_axis", C.c_int32), ("_pad0", C.c_int32),
                ("slope_critical", C.c_double),
                ("step_critical", C.c_double), ("step_radius1", C.c_double), ("step_radius2", C.c_double),
                ("step_ncrit", C.c_int32), ("_pad1", C.c_int32),
                ("rough_critical", C.c_double), ("rough_radius", C.c_double),
                ("w_scale", C.c_float), ("w_slope", C.c_float), ("w_step", C.c_float), ("w_rough", C.c_float),
                ("fp_radius", C.c_double), ("fp_offset", C.c_double), ("fp_default", C.c_double),
                ("fp_max_gap", C.c_double), ("fp_critical_step", C.c_double),
                ("fp_check_roughness", C.c_int32), ("_pad2", C.c_int32)]


class TeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"travgpu error {code}: {msg}")
        self.code = code


_lib = None


def load():
    """dlopen libtravgpu.so.  Raises if it has not been built (no silent fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it with `python -m traversability_estimation_amd.build` "
                              "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        vp, pp = C.c_void_p, C.POINTER(TeParams)
        fp = C.POINTER(C.c_float)
        L.te_params_default.argtypes = [pp]
        L.te_params_validate.argtypes = [pp]
        L.te_device_count.argtypes = [C.POINTER(C.c_int)]
        L.te_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.te_destroy.argtypes = [vp]
        L.te_set_params.argtypes = [vp, pp]
        L.te_get_params.argtypes = [vp, pp]
        L.te_set_option.argtypes = [vp, C.c_int, C.c_int]
        if "TRAVGPU_LIB" not in os.environ or hasattr(L, "te_download_face_flags"):  # (as below: an A/B library of an earlier round)
            L.te_download_face_flags.argtypes = [vp, C.POINTER(C.c_ubyte), C.c_size_t]
        L.te_set_geometry.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double]
        L.te_upload_elevation.argtypes = [vp, fp, C.c_int, C.c_int]
        L.te_upload_tile.argtypes = [vp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        L.te_download_tile.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, fp]
        L.te_upload_tile_async.argtypes = [vp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        L.te_download_tile_async.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, fp]
        L.te_device_ptr.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t)]
        L.te_set_layer_present.argtypes = [vp, C.c_int, C.c_int]
        L.te_upload_layer.argtypes = [vp, C.c_int, fp, C.c_int, C.c_int]
        L.te_upload_layer_circular.argtypes = [vp, C.c_int, fp, C.c_int, C.c_int, C.c_int]
        if "TRAVGPU_LIB" not in os.environ or hasattr(L, "te_prefetch_layers"):  # (an A/B library of an earlier round lacks the pair)
            L.te_prefetch_layers.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(fp)]
            L.te_wait_prefetch.argtypes = [vp]
        L.te_download_layer_circular.argtypes = [vp, C.c_int, fp, C.c_int, C.c_int, C.c_int]
        L.te_run_filter.argtypes = [vp, C.c_int, C.c_uint]
        L.te_run_chain.argtypes = [vp, C.c_uint]
        L.te_run_chain_region.argtypes = [vp, C.c_uint, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        L.te_run_footprint.argtypes = [vp]
        L.te_polygon_untraversable_hull.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_ubyte),
                                                    C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double)]
        L.te_set_check_robot_inclination.argtypes = [vp, C.c_int]
        L.te_check_inclination.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_ubyte), C.POINTER(C.c_int)]
        L.te_check_footprint_paths.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double),
                                               C.POINTER(C.c_ubyte), C.POINTER(C.c_double), C.POINTER(C.c_int)]
        L.te_check_footprint_paths_radius.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double),
                                                      C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_ubyte),
                                                      C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(TePathCheckStats)]
        L.te_run_polygon_footprint.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.c_double]
        L.te_polygons_traversable.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double),
                                              C.POINTER(C.c_ubyte), C.POINTER(C.c_double)]
        L.te_check_polygon_footprint_paths.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int,
                                                       C.POINTER(C.c_double), C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte),
                                                       C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]
        L.te_pin_host.argtypes = [vp, C.c_size_t]
        L.te_unpin_host.argtypes = [vp]
        ip_, dp_ = C.POINTER(C.c_int), C.POINTER(C.c_double)
        L.te_path_polygons.argtypes = [C.c_int, ip_, dp_, C.c_int, dp_, C.POINTER(C.c_ubyte), C.c_int, C.c_int, ip_, ip_, ip_, ip_,
                                       dp_, dp_]
        L.te_sync.argtypes = [vp]
        L.te_download_layer.argtypes = [vp, C.c_int, fp, C.c_int, C.c_int]
        L.te_time_chain.argtypes = [vp, C.c_uint, C.c_int, C.c_int, C.POINTER(C.c_float)]
        L.te_time_chain_samples.argtypes = [vp, C.c_uint, C.c_int, C.c_int, C.POINTER(C.c_float)]
        L.te_shard_range.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.te_bcast_params.argtypes = [C.POINTER(vp), C.c_int, C.c_int]
        L.te_run_chain_multi.argtypes = [C.POINTER(vp), C.c_int, C.c_uint]
        L.te_sync_multi.argtypes = [C.POINTER(vp), C.c_int]
        szp, cpp = C.POINTER(C.c_size_t), C.POINTER(C.c_char_p)
        L.te_msg_parse.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(TeMsgInfo)]
        L.te_msg_layer.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_char_p, szp]
        L.te_msg_write.argtypes = [C.POINTER(TeMsgInfo), C.c_int, cpp, C.POINTER(fp), C.c_int, cpp, vp, C.c_size_t, szp]
        L.te_upload_msg.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_char_p, C.c_int, C.POINTER(TeMsgInfo)]
        L.te_download_msg.argtypes = [vp, C.POINTER(TeMsgInfo), C.c_int, C.POINTER(C.c_int), cpp, C.c_int, cpp, vp,
                                      C.c_size_t, szp]
        L.te_bag_find_message.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, szp, szp]
        L.te_bag_write.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_uint32, C.c_uint32, vp, C.c_size_t, szp]
        L.te_image_parse.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(TeImageInfo), szp]
        L.te_upload_image.argtypes = [vp, C.POINTER(TeImageInfo), vp, C.c_int, C.c_int, C.c_float, C.c_float, C.c_double]
        L.te_upload_image_msg.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_int, C.c_float, C.c_float, C.c_double, C.c_double,
                                          C.c_double, C.c_double, C.POINTER(TeImageInfo)]
        ip, i8p, u32p = C.POINTER(C.c_int), C.POINTER(C.c_int8), C.POINTER(C.c_uint32)
        L.te_download_occupancy.argtypes = [vp, C.c_int, C.c_int, ip, fp, fp, vp]
        L.te_download_occupancy_msg.argtypes = [vp, C.POINTER(TeMsgInfo), C.c_int, C.c_float, C.c_float, vp, C.c_size_t, szp]
        L.te_occupancy_msg_write.argtypes = [C.POINTER(TeOccupancyInfo), i8p, vp, C.c_size_t, szp]
        L.te_occupancy_parse.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(TeOccupancyInfo), szp]
        L.te_download_cloud.argtypes = [vp, C.c_int, C.c_int, ip, C.c_int, C.c_int, ip, vp, C.c_size_t, szp]
        L.te_download_cloud_msg.argtypes = [vp, C.POINTER(TeMsgInfo), C.c_int, ip, cpp, C.c_int, C.c_int, ip, vp, C.c_size_t, szp]
        L.te_cloud_msg_write.argtypes = [C.POINTER(TeCloudInfo), C.c_int, cpp, fp, vp, C.c_size_t, szp]
        L.te_cloud_parse.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(TeCloudInfo), szp]
        L.te_cloud_field.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_char_p, u32p, u32p, u32p]
        L.te_cloud_spans.argtypes = [szp]
        smp = C.POINTER(TeSubmapInfo)
        L.te_submap_geometry.argtypes = [C.c_int, C.c_int] + [C.c_double] * 7 + [smp]
        L.te_download_submap.argtypes = [vp, C.c_int] + [C.c_double] * 4 + [C.c_int, ip, smp, vp, C.c_size_t]
        L.te_download_submap_msg.argtypes = [vp, C.POINTER(TeMsgInfo)] + [C.c_double] * 4 + [C.c_int, ip, cpp, C.c_int, cpp, smp, vp, C.c_size_t, szp]
        if "TRAVGPU_LIB" not in os.environ or hasattr(L, "te_move_map"):  # (an A/B library of an earlier round lacks the pair)
            L.te_move_geometry.argtypes = [C.c_int, C.c_int] + [C.c_double] * 5 + [pp, C.POINTER(TeMoveInfo)]
            L.te_move_map.argtypes = [vp, C.c_double, C.c_double, C.POINTER(TeMoveInfo)]
        L.te_expr_check.argtypes = [C.c_char_p, C.POINTER(TeExprInfo)]
        L.te_run_expression.argtypes = [vp, C.c_char_p, C.c_int]
        L.te_run_expression_region.argtypes = [vp, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        L.te_run_chain_region_expression.argtypes = [vp, C.c_uint, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        L.te_time_expression_samples.argtypes = [vp, C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_float)]
        mp = C.POINTER(TeMedianFillParams)
        L.te_median_fill_params_default.argtypes = [mp]
        L.te_median_fill_params_validate.argtypes = [mp]
        L.te_run_median_fill.argtypes = [vp, mp, C.c_int, C.c_int, C.c_int, C.c_int]
        L.te_upload_layer_tile.argtypes = [vp, C.c_int, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        L.te_run_median_fill_region.argtypes = [vp, mp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
        L.te_run_radius_filter_region.argtypes = [vp, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
        L.te_download_fill_mask.argtypes = [vp, C.c_int, C.POINTER(C.c_ubyte), C.c_size_t]
        L.te_time_median_fill_samples.argtypes = [vp, mp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]
        L.te_run_radius_filter.argtypes = [vp, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int]
        L.te_radius_filter_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.te_time_radius_filter_samples.argtypes = [vp, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]
        L.te_run_distance.argtypes = [vp, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int]
        L.te_run_distance_region.argtypes = [vp, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
        L.te_distance_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.te_time_distance_samples.argtypes = [vp, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]
        L.te_run_components.argtypes = [vp, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        L.te_run_reachable.argtypes = [vp, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
        L.te_components_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
        wp = C.POINTER(TeWindowExprParams)
        L.te_window_expr_params_default.argtypes = [wp]
        L.te_window_expr_params_validate.argtypes = [wp]
        L.te_window_expr_check.argtypes = [C.c_char_p, C.c_int, C.POINTER(TeExprInfo)]
        L.te_run_window_expression.argtypes = [vp, wp, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.te_run_window_expression_region.argtypes = [vp, wp, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
        L.te_window_expression_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.te_time_window_expression_samples.argtypes = [vp, wp, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]
        L.te_add_layer.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int)]
        L.te_remove_layer.argtypes = [vp, C.c_int]
        L.te_layer_id.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int)]
        L.te_layer_name.argtypes = [vp, C.c_int, C.c_char_p, C.c_size_t]
        L.te_expr_check_ctx.argtypes = [vp, C.c_char_p, C.POINTER(TeExprInfo)]
        L.te_run_layer_expression.argtypes = [vp, C.c_char_p, C.c_int]
        L.te_run_layer_expression_region.argtypes = [vp, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        L.te_run_threshold.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int]
        L.te_run_threshold_region.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        L.te_copy_layer.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
        tp = C.POINTER(TeThreshold)
        L.te_run_layer_expression_thresholds.argtypes = [vp, C.c_char_p, C.c_int, C.c_int, tp]
        L.te_run_layer_expression_thresholds_region.argtypes = [vp, C.c_char_p, C.c_int, C.c_int, tp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        L.te_last_error.restype = C.c_char_p
        L.te_version.restype = C.c_char_p
        _lib = L
    return _lib


def _distance_mode(mode, nan_is_seed=False):
    return int(DISTANCE_MODES.get(mode, mode)) | (DISTANCE_NAN_IS_SEED if nan_is_seed else 0)


def _check(rc):
    if rc != TE_OK:
        raise TeError(rc, load().te_last_error().decode())


def default_params(**over):
    p = TeParams()
    _check(load().te_params_default(C.byref(p)))
    for k, v in over.items():
        if not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def default_median_fill_params(**over):
    """te_median_fill_params_default (fill_hole_radius 0.05, no filtering of existing values, 4 opening iterations), then `over`."""
    p = TeMedianFillParams()
    _check(load().te_median_fill_params_default(C.byref(p)))
    for k, v in over.items():
        if not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def window_expr_params(window_size=None, window_length=None, compute_empty_cells=True, edge_handling="inside"):
    """te_window_expr_params from the keys of a SlidingWindowMathExpressionFilter entry: exactly one of window_size (cells) and
    window_length (metres); edge_handling by name or as EDGE_*.  Validated by the library."""
    p = TeWindowExprParams()
    _check(load().te_window_expr_params_default(C.byref(p)))
    p.window_size = 0 if window_size is None else int(window_size)
    p.use_window_length = 0 if window_length is None else 1
    p.window_length = 0.0 if window_length is None else float(window_length)
    if window_size is not None and window_length is not None:
        p.window_length = float(window_length)  # (both given: the library refuses the pair)
    p.compute_empty_cells = 1 if compute_empty_cells else 0
    p.edge_handling = EDGE_HANDLING[edge_handling] if isinstance(edge_handling, str) else int(edge_handling)
    _check(load().te_window_expr_params_validate(C.byref(p)))
    return p


def validate_median_fill_params(p):
    _check(load().te_median_fill_params_validate(C.byref(p)))
    return p


def validate_params(p):
    """The range checks of the reference's configure()s (te_params_validate); raises TeError with the reference's message."""
    _check(load().te_params_validate(C.byref(p)))
    return p


def params_to_bytes(p):
    return bytes(p)


def params_from_bytes(b):
    p = TeParams()
    assert len(b) == C.sizeof(p)
    C.memmove(C.byref(p), b, len(b))
    return p


def _names(names):
    arr = (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
    return arr


def msg_parse(msg):
    """Validate a serialised grid_map_msgs/GridMap; returns (TeMsgInfo, {layer name: byte offset of its payload})."""
    info = TeMsgInfo()
    _check(load().te_msg_parse(msg, len(msg), C.byref(info)))
    layers = {}
    name = C.create_string_buffer(MSG_MAX_NAME)
    off = C.c_size_t()
    for k in range(info.n_layers):
        _check(load().te_msg_layer(msg, len(msg), k, name, C.byref(off)))
        layers[name.value.decode(errors="replace")] = off.value
    return info, layers


def msg_layer(msg, info, offset):
    """The payload at `offset` as a (cols, rows) float32 array in the message's own (circular) storage order."""
    return np.frombuffer(msg, dtype="<f4", count=info.rows * info.cols, offset=offset).reshape(info.cols, info.rows)


def msg_write(info, layers, basic_layers=()):
    """GridMapRosConverter::toMessage for host layers: {name: rows*cols float32 in storage order} -> bytes."""
    names = list(layers)
    arrs = [np.ascontiguousarray(layers[n], dtype=np.float32).reshape(-1) for n in names]
    for a in arrs:
        assert a.size == info.rows * info.cols, (a.size, info.rows, info.cols)
    fpp = C.POINTER(C.c_float)
    data = (fpp * max(len(arrs), 1))(*[a.ctypes.data_as(fpp) for a in arrs])
    need = C.c_size_t()
    L = load()
    L.te_msg_write(C.byref(info), len(names), _names(names), data, len(basic_layers), _names(list(basic_layers)), None, 0,
                   C.byref(need))
    out = C.create_string_buffer(max(need.value, 1))
    _check(L.te_msg_write(C.byref(info), len(names), _names(names), data, len(basic_layers), _names(list(basic_layers)), out,
                          need.value, C.byref(need)))
    return out.raw[:need.value]


def bag_find_message(bag, topic):
    """GridMapRosConverter::loadFromBag's pick: the last grid_map_msgs/GridMap message under `topic`."""
    off, n = C.c_size_t(), C.c_size_t()
    _check(load().te_bag_find_message(bag, len(bag), topic.encode(), C.byref(off), C.byref(n)))
    return bag[off.value:off.value + n.value]


def bag_write(msg, topic, stamp=(0, 0)):
    """GridMapRosConverter::saveToBag: a one-message rosbag V2.0 image."""
    need = C.c_size_t()
    L = load()
    L.te_bag_write(msg, len(msg), topic.encode(), int(stamp[0]), int(stamp[1]), None, 0, C.byref(need))
    out = C.create_string_buffer(max(need.value, 1))
    _check(L.te_bag_write(msg, len(msg), topic.encode(), int(stamp[0]), int(stamp[1]), out, need.value, C.byref(need)))
    return out.raw[:need.value]


def image_parse(msg):
    """Validate a serialised sensor_msgs/Image; returns (TeImageInfo, byte offset of its step * height pixel bytes)."""
    info, off = TeImageInfo(), C.c_size_t()
    _check(load().te_image_parse(msg, len(msg), C.byref(info), C.byref(off)))
    return info, off.value


def occupancy_parse(msg):
    """Validate a serialised nav_msgs/OccupancyGrid; returns (TeOccupancyInfo, byte offset of its width * height cells)."""
    info, off = TeOccupancyInfo(), C.c_size_t()
    _check(load().te_occupancy_parse(msg, len(msg), C.byref(info), C.byref(off)))
    return info, off.value


def occupancy_msg_write(info, data):
    """The message of a TeOccupancyInfo and its width * height int8 cells (host only)."""
    d = np.ascontiguousarray(data, dtype=np.int8).reshape(-1)
    need = C.c_size_t()
    L = load()
    L.te_occupancy_msg_write(C.byref(info), None, None, 0, C.byref(need))
    out = C.create_string_buffer(max(need.value, 1))
    _check(L.te_occupancy_msg_write(C.byref(info), d.ctypes.data_as(C.POINTER(C.c_int8)), out, need.value, C.byref(need)))
    return out.raw[:need.value]


def cloud_parse(msg):
    """Validate a serialised sensor_msgs/PointCloud2; returns (TeCloudInfo, [(name, offset, datatype, count)], byte offset of
    its row_step * height data bytes)."""
    info, off = TeCloudInfo(), C.c_size_t()
    L = load()
    _check(L.te_cloud_parse(msg, len(msg), C.byref(info), C.byref(off)))
    fields = []
    name = C.create_string_buffer(MSG_MAX_NAME)
    o, t, n = C.c_uint32(), C.c_uint32(), C.c_uint32()
    for k in range(info.n_fields):
        _check(L.te_cloud_field(msg, len(msg), k, name, C.byref(o), C.byref(t), C.byref(n)))
        fields.append((name.value.decode(errors="replace"), o.value, t.value, n.value))
    return info, fields, off.value


def cloud_msg_write(info, field_names, points):
    """A cloud of info.width points of len(field_names) float32 fields (host only); points: width x n_fields."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1)
    assert p.size == info.width * len(field_names), (p.size, info.width, len(field_names))
    need = C.c_size_t()
    L = load()
    args = (C.byref(info), len(field_names), _names(list(field_names)), p.ctypes.data_as(C.POINTER(C.c_float)))
    L.te_cloud_msg_write(*args, None, 0, C.byref(need))
    out = C.create_string_buffer(max(need.value, 1))
    _check(L.te_cloud_msg_write(*args, out, need.value, C.byref(need)))
    return out.raw[:need.value]


def cloud_spans():
    """Cells of one wavefront's ballot, of one counting workgroup and of one scan workgroup's span (te_cloud_spans)."""
    c = (C.c_size_t * 3)()
    _check(load().te_cloud_spans(c))
    return tuple(int(v) for v in c)


def submap_geometry(rows, cols, res, pos, position, length):
    """GridMap::getSubmap's geometry for a request (position, length) on a rows x cols map centred at `pos` (host only, no
    context): a TeSubmapInfo -- ok, the rectangle row0 / col0 / rows / cols, the submap's position and length."""
    info = TeSubmapInfo()
    _check(load().te_submap_geometry(int(rows), int(cols), float(res), float(pos[0]), float(pos[1]), float(position[0]),
                                     float(position[1]), float(length[0]), float(length[1]), C.byref(info)))
    return info


def move_geometry(rows, cols, res, pos, new_pos, params=None):
    """te_move_geometry: the plan of moving a rows x cols map held at `pos` to `new_pos` (host only, no context): a TeMoveInfo.
    params=None: results_kept is 0."""
    info = TeMoveInfo()
    _check(load().te_move_geometry(int(rows), int(cols), float(res), float(pos[0]), float(pos[1]), float(new_pos[0]), float(new_pos[1]),
                                   None if params is None else C.byref(params), C.byref(info)))
    return info


def _layer_ids(layers, ctx=None):
    ids = [ctx._lid(v) if ctx is not None else LAYERS[v] if isinstance(v, str) else int(v) for v in layers]
    return (C.c_int * max(len(ids), 1))(*ids), len(ids)


def _image_array(array):
    a = np.asarray(array)
    if a.dtype not in (np.uint8, np.uint16) or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (1, 3, 4)):
        raise ValueError(f"image: H x W or H x W x (1|3|4) of uint8 / uint16, not {a.dtype} {a.shape}")
    return a


def image_msg(array, encoding, step=None, is_bigendian=0, frame_id="map", seq=0, stamp=(0, 0), pad=0xA5):
    """The ROS1 serialisation of a sensor_msgs/Image (pure Python): `array` is H x W or H x W x C of uint8 / uint16 sample
    values, written in the byte order `is_bigendian` names, rows `step` bytes apart (default: packed; the bytes between
    rows are `pad`).  `encoding` is written as given -- also one the parser refuses."""
    a = _image_array(array)
    h, w = a.shape[:2]
    rows = np.ascontiguousarray(a.astype(a.dtype.newbyteorder(">" if is_bigendian else "<"))).view(np.uint8).reshape(h, -1)
    step = rows.shape[1] if step is None else int(step)
    data = np.full((h, max(step, rows.shape[1])), pad, np.uint8)
    data[:, :rows.shape[1]] = rows
    data = data[:, :step].tobytes() if step < rows.shape[1] else data.tobytes()  # (a step below the row: for the parser to refuse)
    f, e = frame_id.encode(), encoding.encode()
    return (struct.pack("<IIII", seq, stamp[0], stamp[1], len(f)) + f + struct.pack("<III", h, w, len(e)) + e +
            struct.pack("<BII", 1 if is_bigendian else 0, step, len(data)) + data)


def pin_host(array):
    """Page-lock a numpy buffer that is reused across frames (te_pin_host); unpin_host before dropping it."""
    _check(load().te_pin_host(array.ctypes.data_as(C.c_void_p), array.nbytes))


def unpin_host(array):
    _check(load().te_unpin_host(array.ctypes.data_as(C.c_void_p)))


def path_polygons(paths, points_xyz, conservative=None):
    """The polygons checkPolygonalFootprintPath evaluates (host computation, no device): returns a list per path of
    (vertices float64[n, 2], area) tuples."""
    paths = [np.asarray(p, dtype=np.float64).reshape(-1, 7) for p in paths]
    n = len(paths)
    off = np.zeros(n + 1, np.int32)
    if n:
        off[1:] = np.cumsum([len(p) for p in paths])
    poses = np.ascontiguousarray(np.concatenate(paths) if n and off[-1] else np.zeros((1, 7)), dtype=np.float64)
    pts = np.ascontiguousarray(points_xyz, dtype=np.float64).reshape(-1, 3)
    cons = None if conservative is None else np.ascontiguousarray(conservative, dtype=np.uint8)
    ip_, dp_ = C.POINTER(C.c_int), C.POINTER(C.c_double)
    args = (n, off.ctypes.data_as(ip_), poses.ctypes.data_as(dp_), len(pts), pts.ctypes.data_as(dp_),
            None if cons is None else cons.ctypes.data_as(C.POINTER(C.c_ubyte)))
    npoly, nvert = C.c_int(), C.c_int()
    L = load()
    L.te_path_polygons(*args, 0, 0, C.byref(npoly), C.byref(nvert), None, None, None, None)  # sizing call
    first = np.zeros(n + 1, np.int32)
    voff = np.zeros(npoly.value + 1, np.int32)
    xy = np.zeros((max(nvert.value, 1), 2), np.float64)
    area = np.zeros(max(npoly.value, 1), np.float64)
    _check(L.te_path_polygons(*args, npoly.value, nvert.value, C.byref(npoly), C.byref(nvert), first.ctypes.data_as(ip_),
                              voff.ctypes.data_as(ip_), xy.ctypes.data_as(dp_), area.ctypes.data_as(dp_)))
    return [[(xy[voff[q]:voff[q + 1]].copy(), float(area[q])) for q in range(first[k], first[k + 1])] for k in range(n)]


def expr_check(text):
    """te_expr_check: compiles a MathExpressionFilter expression on the host (no device, no context).  Returns
    {"n_instructions", "layers" (names, in te_layer order), "n_reductions", "stack_depth"}; raises TeError with the library's
    message and class (TE_ERR_BAD_PARAM: not an expression of the language; TE_ERR_UNSUPPORTED: valid EigenLab that is not built)."""
    info = TeExprInfo()
    _check(load().te_expr_check(str(text).encode(), C.byref(info)))
    return {"n_instructions": int(info.n_instructions), "layers": [k for k, v in LAYERS.items() if info.layer_mask >> v & 1],
            "n_reductions": int(info.n_reductions), "stack_depth": int(info.stack_depth)}


def window_expr_check(text, in_layer="elevation"):
    """te_window_expr_check: compiles a SlidingWindowMathExpressionFilter expression over `in_layer` on the host (no device, no
    context).  Returns what expr_check returns; raises TeError with the library's message (it names the column) and class."""
    info = TeExprInfo()
    lid = LAYERS[in_layer] if isinstance(in_layer, str) else int(in_layer)
    _check(load().te_window_expr_check(str(text).encode(), lid, C.byref(info)))
    return {"n_instructions": int(info.n_instructions), "layers": [k for k, v in LAYERS.items() if info.layer_mask >> v & 1],
            "n_reductions": int(info.n_reductions), "stack_depth": int(info.stack_depth)}


def device_count():
    n = C.c_int(0)
    rc = load().te_device_count(C.byref(n))
    return n.value if rc == TE_OK else 0


class Context:
    """One device context: owns the device-resident layers of a batch of maps (thin OO view of te_ctx)."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        _check(load().te_create(int(device), C.byref(self._h)))
        self.rows = self.cols = self.batch = 0

    def close(self):
        if self._h:
            load().te_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_params(self, p):
        _check(load().te_set_params(self._h, C.byref(p)))

    def set_option(self, option, value):
        _check(load().te_set_option(self._h, int(option), int(value)))

    def download_face_flags(self):
        """(batch, ceil(cols / 4), ceil(rows / 64)) uint8: the face flags a footprint run would be given now."""
        out = np.empty((self.batch, (self.cols + 3) // 4, (self.rows + 63) // 64), np.uint8)
        _check(load().te_download_face_flags(self._h, out.ctypes.data_as(C.POINTER(C.c_ubyte)), out.size))
        return out

    def get_params(self):
        p = TeParams()
        _check(load().te_get_params(self._h, C.byref(p)))
        return p

    def set_geometry(self, rows, cols, batch, res, pos=(0.0, 0.0)):
        _check(load().te_set_geometry(self._h, int(rows), int(cols), int(batch), float(res), float(pos[0]), float(pos[1])))
        self.rows, self.cols, self.batch = int(rows), int(cols), int(batch)

    def upload_elevation(self, elev, map0=0):
        a = np.ascontiguousarray(elev, dtype=np.float32).reshape(-1)
        per = self.rows * self.cols
        assert a.size % per == 0, (a.size, per)
        _check(load().te_upload_elevation(self._h, a.ctypes.data_as(C.POINTER(C.c_float)), int(map0), a.size // per))

    def upload_tile(self, tile, map_index, row0, col0):
        """tile: array of shape (w, h) == [col][row] (column-major h x w tile)."""
        t = np.ascontiguousarray(tile, dtype=np.float32)
        w, h = t.shape
        _check(load().te_upload_tile(self._h, t.ctypes.data_as(C.POINTER(C.c_float)), int(map_index), int(row0),
                                     int(col0), int(h), int(w)))

    def download_tile(self, layer, map_index, row0, col0, h, w):
        """The h x w rectangle of a layer as an array of shape (w, h) == [col][row]."""
        t = np.empty((int(w), int(h)), np.float32)
        _check(load().te_download_tile(self._h, self._lid(layer), int(map_index), int(row0),
                                       int(col0), int(h), int(w), t.ctypes.data_as(C.POINTER(C.c_float))))
        return t

    def upload_tile_async(self, tile, map_index, row0, col0):
        """As upload_tile, but returns at once (copy-in stream + staging slot); `tile` must be a C-contiguous float32 array of
        shape (w, h) that stays alive and unchanged until sync() -- page-lock it (pin_host) for a truly asynchronous copy."""
        assert tile.dtype == np.float32 and tile.flags["C_CONTIGUOUS"], "upload_tile_async: float32, C-contiguous (no hidden copy)"
        w, h = tile.shape
        _check(load().te_upload_tile_async(self._h, tile.ctypes.data_as(C.POINTER(C.c_float)), int(map_index), int(row0), int(col0),
                                           int(h), int(w)))

    def download_tile_async(self, layer, map_index, row0, col0, out):
        """The rectangle of shape out.shape == (w, h) into `out` (float32, C-contiguous); valid after sync()."""
        assert out.dtype == np.float32 and out.flags["C_CONTIGUOUS"]
        w, h = out.shape
        _check(load().te_download_tile_async(self._h, self._lid(layer), int(map_index),
                                             int(row0), int(col0), int(h), int(w), out.ctypes.data_as(C.POINTER(C.c_float))))

    def device_ptr(self, layer):
        p, n = C.c_void_p(), C.c_size_t()
        _check(load().te_device_ptr(self._h, self._lid(layer), C.byref(p),
                                    C.byref(n)))
        return p.value, n.value

    def set_layer_present(self, layer, present):
        _check(load().te_set_layer_present(self._h, self._lid(layer), 1 if present else 0))

    def upload_layer(self, layer, data, map0=0):
        a = np.ascontiguousarray(data, dtype=np.float32).reshape(-1)
        per = self.rows * self.cols
        assert a.size % per == 0, (a.size, per)
        _check(load().te_upload_layer(self._h, self._lid(layer),
                                      a.ctypes.data_as(C.POINTER(C.c_float)), int(map0), a.size // per))

    def upload_layer_tile(self, layer, tile, map_index, row0, col0):
        """upload_tile for any layer that has memory (te_upload_layer_tile); tile: array of shape (w, h) == [col][row]."""
        t = np.ascontiguousarray(tile, dtype=np.float32)
        w, h = t.shape
        _check(load().te_upload_layer_tile(self._h, self._lid(layer), t.ctypes.data_as(C.POINTER(C.c_float)),
                                           int(map_index), int(row0), int(col0), int(h), int(w)))

    def prefetch_layers(self, layers):
        """{layer: array}: whole-layer uploads that run beside the calls that follow, until wait_prefetch() (te_prefetch_layers).
        The arrays are kept alive by this object until then."""
        names = list(layers)
        arrs = [np.ascontiguousarray(layers[k], dtype=np.float32).reshape(-1) for k in names]
        for a in arrs:
            assert a.size == self.rows * self.cols * self.batch, (a.size, self.rows, self.cols, self.batch)
        ids = (C.c_int * len(names))(*[self._lid(k) for k in names])
        ptrs = (C.POINTER(C.c_float) * len(names))(*[a.ctypes.data_as(C.POINTER(C.c_float)) for a in arrs])
        self._prefetch_keep = arrs
        _check(load().te_prefetch_layers(self._h, len(names), ids, ptrs))

    def wait_prefetch(self):
        try:
            _check(load().te_wait_prefetch(self._h))
        finally:
            self._prefetch_keep = None

    def upload_layer_circular(self, layer, data, start_index, map_index=0):
        """Upload ONE map's layer given in GridMap buffer order (start_index = GridMap::getStartIndex())."""
        a = np.ascontiguousarray(data, dtype=np.float32).reshape(-1)
        assert a.size == self.rows * self.cols, (a.size, self.rows, self.cols)
        _check(load().te_upload_layer_circular(self._h, self._lid(layer),
                                               a.ctypes.data_as(C.POINTER(C.c_float)), int(map_index),
                                               int(start_index[0]), int(start_index[1])))

    def download_layer_circular(self, layer, start_index, map_index=0):
        """Download ONE map's layer into GridMap buffer order; returns a (cols, rows) array (row index fastest)."""
        out = np.empty((self.cols, self.rows), dtype=np.float32)
        _check(load().te_download_layer_circular(self._h, self._lid(layer),
                                                 out.ctypes.data_as(C.POINTER(C.c_float)), int(map_index),
                                                 int(start_index[0]), int(start_index[1])))
        return out

    def run_filter(self, which, flags=0):
        _check(load().te_run_filter(self._h, FILTERS[which] if isinstance(which, str) else int(which), int(flags)))

    def run_chain(self, flags=0):
        _check(load().te_run_chain(self._h, int(flags)))

    def run_chain_region(self, map_index, row0, col0, h, w, flags=0):
        _check(load().te_run_chain_region(self._h, int(flags), int(map_index), int(row0), int(col0), int(h), int(w)))

    def run_footprint(self):
        _check(load().te_run_footprint(self._h))

    def move_map(self, x, y):
        """te_move_map: GridMap::move of every resident layer to the position (x, y), rounded to whole cells; asynchronous like
        run_chain.  Returns the TeMoveInfo: hand it to refresh_moved."""
        info = TeMoveInfo()
        _check(load().te_move_map(self._h, float(x), float(y), C.byref(info)))
        return info

    def refresh_moved(self, info, flags=0, tiles=None, map_index=0, expression=None):
        """The loop a caller writes after move_map, for one map: for each rectangle of `info`, upload its tile if the rectangle
        is exposed and a tile is given (tiles[k]: the array of shape (w, h) for rectangle k, or None), then run_chain_region on
        it -- trailing lines included.  With results_kept == 0 (a tie radius, raster normals) the tiles are uploaded and the
        whole chain runs instead.  A zero-shift move has nothing to refresh.
        The footprint flags are served by ONE whole-map footprint pass behind the region runs, not by the region runs: the
        footprint checks' own windows, circle(3 res) and circle(2.5 res), have cells on their circle at every resolution, so
        the untraversable mask is decided anew at the new position (include/travgpu.h, caveat 3).
        expression: the combined layer is this text (run_expression) instead of the weighted sum -- the region runs are
        run_chain_region_expression, and a whole chain is followed by run_expression before the footprint pass."""
        rects = info.rectangles()
        fp = flags & (RUN_FOOTPRINT | RUN_FOOTPRINT_MEMO)
        for k, ((row0, col0, h, w), exposed) in enumerate(rects):
            if exposed and tiles is not None and tiles[k] is not None:
                self.upload_tile(tiles[k], map_index, row0, col0)
            if info.results_kept:
                self.run_chain_region_expression(expression, map_index, row0, col0, h, w, flags & ~fp)
        if rects and not info.results_kept:
            self.run_chain(flags if expression is None else flags & ~fp)
            if expression is not None:
                self.run_expression(expression)
                if fp:
                    self.run_footprint()
        elif rects and fp:
            self.run_footprint()

    def run_expression(self, text, out="traversability"):
        """te_run_expression: `out` = text over the resident layers (any MathExpressionFilter expression of the language in
        include/travgpu.h); asynchronous like run_chain.  The context is then what upload_layer(out, the same values) leaves."""
        _check(load().te_run_expression(self._h, str(text).encode(), self._lid(out)))

    def run_expression_region(self, text, map_index, row0, col0, h, w, out="traversability"):
        """te_run_expression_region: `out` = text on the cells of the rectangle of one map, the bits of run_expression; a text
        with a reduction or one that reads `out` is refused (TE_ERR_UNSUPPORTED).  The context is then what
        upload_layer_tile(out, the same values) leaves."""
        _check(load().te_run_expression_region(self._h, str(text).encode(), self._lid(out), int(map_index), int(row0),
                                               int(col0), int(h), int(w)))

    # ---- user layers, expressions over any layer, ThresholdFilter / DuplicationFilter (include/travgpu.h) ----
    def _lid(self, layer):
        """The id of a layer given by its name (a reference name, or a user layer of this context) or by its id."""
        if not isinstance(layer, str):
            return int(layer)
        return LAYERS[layer] if layer in LAYERS else self.layer_id(layer)

    def add_layer(self, name):
        """te_add_layer: a user layer under `name` (an existing one: its id); returns the id."""
        lid = C.c_int(-1)
        _check(load().te_add_layer(self._h, str(name).encode(), C.byref(lid)))
        return lid.value

    def remove_layer(self, layer):
        """te_remove_layer (gridMapFilters/DeletionFilter): frees the memory and the name of a user layer."""
        _check(load().te_remove_layer(self._h, self._lid(layer)))

    def layer_id(self, name):
        lid = C.c_int(-1)
        _check(load().te_layer_id(self._h, str(name).encode(), C.byref(lid)))
        return lid.value

    def layer_name(self, layer):
        buf = C.create_string_buffer(MSG_MAX_NAME)
        _check(load().te_layer_name(self._h, int(layer), buf, len(buf)))
        return buf.value.decode()

    def expr_check(self, text):
        """te_expr_check_ctx: expr_check with this context's user layers as operands; "layers" holds their names too."""
        info = TeExprInfo()
        _check(load().te_expr_check_ctx(self._h, str(text).encode(), C.byref(info)))
        return {"n_instructions": int(info.n_instructions), "layers": [self.layer_name(k) for k in range(32) if info.layer_mask >> k & 1],
                "n_reductions": int(info.n_reductions), "stack_depth": int(info.stack_depth), "layer_mask": int(info.layer_mask)}

    @staticmethod
    def _thresholds(thresholds):
        """[(mode, threshold, set_to), ...] with mode "lower" / "upper" (or TE_THRESHOLD_*) as a te_threshold array."""
        arr = (TeThreshold * max(len(thresholds), 1))()
        for k, (mode, thr, set_to) in enumerate(thresholds):
            arr[k].mode = THRESHOLD_MODES[mode] if isinstance(mode, str) else int(mode)
            arr[k].threshold, arr[k].set_to = float(thr), float(set_to)
        return arr, len(thresholds)

    def run_layer_expression(self, text, out, thresholds=None):
        """te_run_layer_expression: `out` (any layer, user layers included) = text.  thresholds: ThresholdFilters on `out`
        fused into the same launch (te_run_layer_expression_thresholds), the bits of run_threshold behind the expression."""
        if thresholds is None:
            _check(load().te_run_layer_expression(self._h, str(text).encode(), self._lid(out)))
        else:
            arr, n = self._thresholds(thresholds)
            _check(load().te_run_layer_expression_thresholds(self._h, str(text).encode(), self._lid(out), n, arr))

    def run_layer_expression_region(self, text, out, map_index, row0, col0, h, w, thresholds=None):
        rect = (int(map_index), int(row0), int(col0), int(h), int(w))
        if thresholds is None:
            _check(load().te_run_layer_expression_region(self._h, str(text).encode(), self._lid(out), *rect))
        else:
            arr, n = self._thresholds(thresholds)
            _check(load().te_run_layer_expression_thresholds_region(self._h, str(text).encode(), self._lid(out), n, arr, *rect))

    def run_threshold(self, layer, mode, threshold, set_to, map0=0, nmaps=None):
        """gridMapFilters/ThresholdFilter in place (te_run_threshold): mode "lower": v < threshold ? set_to : v; "upper": v > threshold."""
        nmaps = self.batch - map0 if nmaps is None else nmaps
        m = THRESHOLD_MODES[mode] if isinstance(mode, str) else int(mode)
        _check(load().te_run_threshold(self._h, self._lid(layer), m, float(threshold), float(set_to), int(map0), int(nmaps)))

    def run_threshold_region(self, layer, mode, threshold, set_to, map_index, row0, col0, h, w):
        m = THRESHOLD_MODES[mode] if isinstance(mode, str) else int(mode)
        _check(load().te_run_threshold_region(self._h, self._lid(layer), m, float(threshold), float(set_to), int(map_index), int(row0), int(col0),
                                              int(h), int(w)))

    def copy_layer(self, src, dst, map0=0, nmaps=None):
        """gridMapFilters/DuplicationFilter (te_copy_layer): dst = src, a copy on the device."""
        nmaps = self.batch - map0 if nmaps is None else nmaps
        _check(load().te_copy_layer(self._h, self._lid(src), self._lid(dst), int(map0), int(nmaps)))

    def run_filter_chain(self, steps, input_layer="elevation", fuse=True):
        """Runs the steps of params_yaml.filter_chain_from_yaml in file order on the context's stream and returns the C-ABI calls
        it made as a list of (name, arguments).  Layers the file names that are not the reference's are added (te_add_layer);
        DeletionFilter removes the user layers it names (the normal layers need no call: the next chain rewrites them).
        NormalVectorsFilter, SlopeFilter, StepFilter, RoughnessFilter run as the individual plugins (te_run_filter) with the
        parameters of their entries, and a MathExpressionFilter that is the weighted sum of the three scores into
        `traversability` as TE_FILTER_COMBINE; the plugins read `input_layer`, which must be the elevation layer.
        fuse (the default: measured 0.108 ms against 0.136 ms for an expression with two thresholds at 4096^2,
        profiles/filter_chain_bench.json): a MathExpressionFilter and the ThresholdFilters that directly follow on its output
        layer are one launch (params_yaml.plan_filter_chain); where the text with its thresholds no longer fits the 64
        instructions the calls are issued one by one."""
        from . import params_yaml as Y
        calls = []

        def call(name, fn, *args):
            fn(*args)
            calls.append((name, args))

        def known(name):
            if name not in LAYERS:
                try:
                    self.layer_id(name)
                except TeError:
                    call("te_add_layer", self.add_layer, name)
            return name

        plugins = [s for s in steps if "fields" in s]
        weighted = {}
        for s in steps:
            if s["filter"] == "expression" and s["output_layer"] == "traversability":
                try:
                    weighted[id(s)] = {k: float(v) for k, v in Y.parse_weighted_sum(s["expression"]).items()}
                except Y.ParamsYamlError:
                    pass
        if plugins and input_layer != "elevation":
            raise ValueError("run_filter_chain: the plugin filters read the elevation layer (input_layer=%r)" % (input_layer,))
        if len(weighted) > 1 and len({tuple(sorted(w.items())) for w in weighted.values()}) > 1:
            weighted = {}  # (several weighted sums with different weights: they run as general expressions)
        applied = {}

        def apply(fields):
            if any(applied.get(k) != v for k, v in fields.items()):
                p = self.get_params()
                for k, v in fields.items():
                    setattr(p, k, v)
                call("te_set_params", self.set_params, p)
                calls[-1] = ("te_set_params", tuple(sorted(fields.items())))
                applied.update(fields)

        merged = {}
        for f in [s["fields"] for s in plugins] + list(weighted.values()):
            for k, v in f.items():
                if merged.setdefault(k, v) != v:
                    merged = None
                    break
            if merged is None:
                break
        if merged:
            apply(merged)
        for kind, s, fused in Y.plan_filter_chain(steps, fuse):
            if kind == "median_fill":
                call("te_run_median_fill", self.run_median_fill, default_median_fill_params(**s["params"]), known(s["input_layer"]), known(s["output_layer"]))
                calls[-1] = ("te_run_median_fill", (tuple(sorted(s["params"].items())), s["input_layer"], s["output_layer"]))
            elif kind == "radius":
                call("te_run_radius_filter", self.run_radius_filter, RADIUS_MEAN if s["op"] == "mean" else RADIUS_MIN, s["radius"], known(s["input_layer"]),
                     known(s["output_layer"]))
            elif kind == "window_expression":
                call("te_run_window_expression", self.run_window_expression, s["expression"], window_expr_params(**s["params"]), known(s["input_layer"]),
                     known(s["output_layer"]))
                calls[-1] = ("te_run_window_expression", (s["expression"], tuple(sorted(s["params"].items())), s["input_layer"], s["output_layer"]))
            elif kind in ("normals", "slope", "step", "roughness"):
                apply(s["fields"])
                if kind == "normals":
                    call("te_set_option", self.set_option, OPT_NORMALS_ALGORITHM, 1 if s["algorithm"] == "raster" else 0)
                call("te_run_filter", self.run_filter, kind)
            elif kind == "expression":
                steps_t = [(t["mode"], t["threshold"], t["set_to"]) for t in fused]
                out = known(s["output_layer"])
                if id(s) in weighted and not fused:
                    apply(weighted[id(s)])
                    call("te_run_filter", self.run_filter, "combine")
                    continue
                if fused and self.expr_check(s["expression"])["n_instructions"] + len(fused) <= 64:
                    call("te_run_layer_expression_thresholds", self.run_layer_expression, s["expression"], out, steps_t)
                    continue
                call("te_run_layer_expression", self.run_layer_expression, s["expression"], out)
                for t in steps_t:
                    call("te_run_threshold", self.run_threshold, out, *t)
            elif kind == "threshold":
                call("te_run_threshold", self.run_threshold, known(s["layer"]), s["mode"], s["threshold"], s["set_to"])
            elif kind == "duplication":
                call("te_copy_layer", self.copy_layer, known(s["input_layer"]), known(s["output_layer"]))
            elif kind == "deletion":
                for name in s["layers"]:
                    if name not in LAYERS:
                        call("te_remove_layer", self.remove_layer, name)
            else:
                raise ValueError("run_filter_chain: unknown step %r" % (kind,))
        return calls

    def run_chain_region_expression(self, text, map_index, row0, col0, h, w, flags=0):
        """te_run_chain_region_expression: run_chain_region with `text` in the place of the weighted sum on the rectangle the
        chain recombines, the footprint half (flags) behind it: the whole tick in one call.  text=None: run_chain_region."""
        _check(load().te_run_chain_region_expression(self._h, int(flags), None if text is None else str(text).encode(), int(map_index), int(row0),
                                                     int(col0), int(h), int(w)))

    def run_median_fill(self, params=None, layer="elevation", out=None, map0=0, nmaps=None):
        """gridMapFilters/MedianFillFilter on the device (te_run_median_fill): `out` (default: `layer`, in place) = the filled `layer`."""
        p = default_median_fill_params() if params is None else params
        lid = lambda name: self._lid(name)
        nmaps = self.batch - map0 if nmaps is None else nmaps
        _check(load().te_run_median_fill(self._h, C.byref(p), lid(layer), lid(layer if out is None else out), int(map0), int(nmaps)))

    def run_median_fill_region(self, params, layer, out, map_index, row0, col0, h, w):
        """te_run_median_fill_region: `out` = the fill of `layer` after it changed inside the rectangle only; `out` held the fill of
        the earlier contents.  Returns (row0, col0, h, w) of the rectangle written."""
        p = default_median_fill_params() if params is None else params
        lid = lambda name: self._lid(name)
        rect = (C.c_int * 4)()
        _check(load().te_run_median_fill_region(self._h, C.byref(p), lid(layer), lid(out), int(map_index), int(row0), int(col0), int(h), int(w), rect))
        return tuple(int(v) for v in rect)

    def download_fill_mask(self, map_index=0):
        """(cols, rows) uint8: shouldFill of the last run_median_fill that covered the map."""
        out = np.empty((self.cols, self.rows), np.uint8)
        _check(load().te_download_fill_mask(self._h, int(map_index), out.ctypes.data_as(C.POINTER(C.c_ubyte)), out.size))
        return out

    def time_median_fill_samples(self, params, layer="elevation", out="traversability_roughness", warmup=3, iters=50):
        """Device time of each of `iters` fills (params=None: device copies of the layer, the fill's floor), in ms."""
        return self._time_samples(load().te_time_median_fill_samples, (None if params is None else C.byref(params),), layer, out, warmup, iters)

    def _time_samples(self, entry, args, in_layer, out_layer, warmup, iters):
        """te_time_*_samples of a layer filter: `args` are what it takes between the context and the two layers."""
        ms = (C.c_float * int(iters))()
        _check(entry(self._h, *args, LAYERS[in_layer], LAYERS[out_layer], int(warmup), int(iters), ms))
        return np.array(ms[:], dtype=np.float64)

    def _block_counts(self, entry):
        counts = (C.c_uint64 * 2)()
        _check(entry(self._h, counts))
        return int(counts[0]), int(counts[1])

    def run_radius_filter(self, op, radius, in_layer="elevation", out_layer=None, map0=0, nmaps=None):
        """gridMapFilters/MeanInRadiusFilter (op RADIUS_MEAN or "mean") / MinInRadiusFilter (RADIUS_MIN, "min") on the device
        (te_run_radius_filter): `out_layer` (default: `in_layer`, in place) = the mean / minimum of `in_layer` within `radius`."""
        op = {"mean": RADIUS_MEAN, "min": RADIUS_MIN}.get(op, op)
        lid = lambda name: self._lid(name)
        nmaps = self.batch - map0 if nmaps is None else nmaps
        _check(load().te_run_radius_filter(self._h, int(op), float(radius), lid(in_layer), lid(in_layer if out_layer is None else out_layer),
                                           int(map0), int(nmaps)))

    def run_radius_filter_region(self, op, radius, in_layer, out_layer, map_index, row0, col0, h, w):
        """te_run_radius_filter_region: `out_layer` = the mean / minimum of `in_layer` after it changed inside the rectangle only.
        Returns (row0, col0, h, w) of the rectangle written."""
        op = {"mean": RADIUS_MEAN, "min": RADIUS_MIN}.get(op, op)
        lid = lambda name: self._lid(name)
        rect = (C.c_int * 4)()
        _check(load().te_run_radius_filter_region(self._h, int(op), float(radius), lid(in_layer), lid(out_layer), int(map_index), int(row0), int(col0),
                                                  int(h), int(w), rect))
        return tuple(int(v) for v in rect)

    def radius_filter_stats(self):
        """(workgroups the sliding kernel settled, workgroups the in-order gather settled) of the last run_radius_filter."""
        return self._block_counts(load().te_radius_filter_stats)

    def time_radius_filter_samples(self, op, radius, in_layer="elevation", out_layer="traversability_roughness", warmup=3, iters=50):
        """Device time of each of `iters` radius filters (op 0: device copies of the layer), in ms."""
        return self._time_samples(load().te_time_radius_filter_samples, (int(op), float(radius)), in_layer, out_layer, warmup, iters)

    def run_distance(self, mode, threshold, max_distance, in_layer="traversability", out_layer=None, map0=0, nmaps=None, nan_is_seed=False):
        """The clearance layer (te_run_distance): `out_layer` (default: `in_layer`, in place) = the exact distance in metres of every
        cell of `in_layer` to the nearest seed of its map -- a cell below (mode DISTANCE_BELOW or "below") or above (DISTANCE_ABOVE,
        "above") `threshold`, with nan_is_seed (or DISTANCE_NAN_IS_SEED or-ed into the mode) a NaN cell too -- capped at `max_distance`."""
        lid = lambda name: self._lid(name)
        nmaps = self.batch - map0 if nmaps is None else nmaps
        _check(load().te_run_distance(self._h, _distance_mode(mode, nan_is_seed), float(threshold), float(max_distance), lid(in_layer),
                                      lid(in_layer if out_layer is None else out_layer), int(map0), int(nmaps)))

    def run_distance_region(self, mode, threshold, max_distance, in_layer, out_layer, map_index, row0, col0, h, w, nan_is_seed=False):
        """te_run_distance_region: `out_layer` = the distance layer of `in_layer` after it changed inside the rectangle only.
        Returns (row0, col0, h, w) of the rectangle written: the given one grown by the cap in cells."""
        lid = lambda name: self._lid(name)
        rect = (C.c_int * 4)()
        _check(load().te_run_distance_region(self._h, _distance_mode(mode, nan_is_seed), float(threshold), float(max_distance), lid(in_layer), lid(out_layer),
                                             int(map_index), int(row0), int(col0), int(h), int(w), rect))
        return tuple(int(v) for v in rect)

    def distance_stats(self):
        """(workgroups of the second pass on the tiled route, on the route of any reach) of the last run_distance(_region)."""
        return self._block_counts(load().te_distance_stats)

    def time_distance_samples(self, mode, threshold, max_distance, in_layer="traversability", out_layer="traversability_roughness", warmup=3, iters=50):
        """Device time of each of `iters` distance layers (mode 0: device copies of the layer; DISTANCE_TIME_PASS1 / _PASS2 or-ed in:
        that pass alone), in ms."""
        return self._time_samples(load().te_time_distance_samples, (int(mode), float(threshold), float(max_distance)), in_layer, out_layer, warmup, iters)

    def run_components(self, mode, threshold, connectivity=4, in_layer="traversability", out_layer=None, map0=0, nmaps=None, nan_is_seed=False):
        """Connected regions (te_run_components): `out_layer` (default: `in_layer`, in place) = for every free cell of `in_layer` the
        number of cells of its component under `connectivity` (4 or 8), 0 for a blocked cell.  Blocked: a seed of run_distance under
        the same mode ("below" / "above"), threshold and nan_is_seed."""
        lid = lambda name: self._lid(name)
        nmaps = self.batch - map0 if nmaps is None else nmaps
        _check(load().te_run_components(self._h, _distance_mode(mode, nan_is_seed), float(threshold), int(connectivity), lid(in_layer),
                                        lid(in_layer if out_layer is None else out_layer), int(map0), int(nmaps)))

    def run_reachable(self, mode, threshold, starts, connectivity=4, in_layer="traversability", out_layer=None, map_index=0, nan_is_seed=False):
        """te_run_reachable: `out_layer` (default: `in_layer`, in place) = 1 on every free cell of map `map_index` connected to one of
        `starts` = [(row, col), ...], 0 on every other cell."""
        lid = lambda name: self._lid(name)
        flat = [int(v) for rc in starts for v in rc]
        if len(flat) != 2 * len(starts):
            raise ValueError("starts must be (row, col) pairs")
        cells = (C.c_int * max(1, len(flat)))(*flat)
        _check(load().te_run_reachable(self._h, _distance_mode(mode, nan_is_seed), float(threshold), int(connectivity), lid(in_layer),
                                       lid(in_layer if out_layer is None else out_layer), int(map_index), len(starts), cells))

    def components_stats(self):
        """(components, free cells, cells of the largest component, cells written 1.0) of the last run_components / run_reachable,
        over all its maps; read from the device (waits for the stream)."""
        counts = (C.c_uint64 * 4)()
        _check(load().te_components_stats(self._h, counts))
        return tuple(int(v) for v in counts)

    def run_window_expression(self, text, params, in_layer="elevation", out_layer=None, map0=0, nmaps=None):
        """gridMapFilters/SlidingWindowMathExpressionFilter on the device (te_run_window_expression): `out_layer` (default:
        `in_layer`, in place) = `text` over the window of every cell of `in_layer`.  params: window_expr_params(...), or a dict of
        its arguments."""
        p = window_expr_params(**params) if isinstance(params, dict) else params
        lid = lambda name: self._lid(name)
        nmaps = self.batch - map0 if nmaps is None else nmaps
        _check(load().te_run_window_expression(self._h, C.byref(p), str(text).encode(), lid(in_layer),
                                               lid(in_layer if out_layer is None else out_layer), int(map0), int(nmaps)))

    def run_window_expression_region(self, text, params, in_layer, out_layer, map_index, row0, col0, h, w):
        """te_run_window_expression_region: `out_layer` = the window expression of `in_layer` after it changed inside the rectangle
        only; `out_layer` held the expression of the earlier contents.  Returns (row0, col0, h, w) of the rectangle written."""
        p = window_expr_params(**params) if isinstance(params, dict) else params
        lid = lambda name: self._lid(name)
        rect = (C.c_int * 4)()
        _check(load().te_run_window_expression_region(self._h, C.byref(p), str(text).encode(), lid(in_layer), lid(out_layer), int(map_index), int(row0),
                                                      int(col0), int(h), int(w), rect))
        return tuple(int(v) for v in rect)

    def window_expression_stats(self):
        """(workgroups the separable route settled, workgroups that walked directly) of the last run_window_expression."""
        return self._block_counts(load().te_window_expression_stats)

    def time_window_expression_samples(self, text, params, in_layer="elevation", out_layer="traversability_roughness", warmup=3, iters=50):
        """Device time of each of `iters` window expressions (text=None: device copies of the layer), in ms."""
        args = (None, None) if text is None else (C.byref(params), str(text).encode())
        return self._time_samples(load().te_time_window_expression_samples, args, in_layer, out_layer, warmup, iters)

    def time_expression_samples(self, text, warmup=3, iters=50):
        """Device ms of `iters` run_expression(text) launches, one event pair each; text=None times run_filter("combine")."""
        ms = (C.c_float * int(iters))()
        _check(load().te_time_expression_samples(self._h, None if text is None else str(text).encode(), int(warmup), int(iters), ms))
        return np.array(ms[:], dtype=np.float64)

    def check_footprint_paths(self, paths, map_index=0):
        """paths: sequence of (n_i, 2) arrays of (x, y) poses.  Returns (is_safe[bool], traversability[float64], status[int32])
        like TraversabilityMap::checkFootprintPath for circular footprints, on the resident footprint layer."""
        off, xy = pack_paths(paths)
        return self.check_footprint_paths_packed(off, xy, map_index)

    def check_footprint_paths_packed(self, off, xy, map_index=0):
        """The same with the poses already packed: off int32[n+1] (off[0] == 0), xy float64[off[-1], 2]."""
        off = np.ascontiguousarray(off, dtype=np.int32)
        xy = np.ascontiguousarray(xy, dtype=np.float64)
        n = len(off) - 1
        safe = np.zeros(max(n, 1), np.uint8)
        trav = np.zeros(max(n, 1), np.float64)
        st = np.zeros(max(n, 1), np.int32)
        _check(load().te_check_footprint_paths(self._h, int(map_index), n, off.ctypes.data_as(C.POINTER(C.c_int)),
                                               xy.ctypes.data_as(C.POINTER(C.c_double)),
                                               safe.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                               trav.ctypes.data_as(C.POINTER(C.c_double)),
                                               st.ctypes.data_as(C.POINTER(C.c_int))))
        return safe[:n].astype(bool), trav[:n], st[:n]

    def check_footprint_paths_radius(self, paths, radii, offset=0.15, map_index=0, want_stats=False):
        """checkFootprintPath for circular footprints with every path at its own radius (FootprintPath.radius), evaluated on
        demand at the centres the paths visit: no footprint layer is needed, read or written (te_check_footprint_paths_radius).
        radii: a scalar, or one value per path.  Returns (is_safe, traversability, status), and with want_stats a dict
        n_visits / n_discs / n_radius_classes as the fourth element."""
        off, xy = pack_paths(paths)
        n = len(off) - 1
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(radii, dtype=np.float64), (n,)) if np.ndim(radii) == 0
                                 else np.asarray(radii, dtype=np.float64).reshape(-1))
        if len(r) != n:
            raise ValueError(f"{len(r)} radii for {n} paths")
        if n == 0:
            r = np.zeros(1, np.float64)
        safe = np.zeros(max(n, 1), np.uint8)
        trav = np.zeros(max(n, 1), np.float64)
        st = np.zeros(max(n, 1), np.int32)
        stats = TePathCheckStats()
        dp = C.POINTER(C.c_double)
        _check(load().te_check_footprint_paths_radius(self._h, int(map_index), n, off.ctypes.data_as(C.POINTER(C.c_int)),
                                                      xy.ctypes.data_as(dp), r.ctypes.data_as(dp), float(offset),
                                                      safe.ctypes.data_as(C.POINTER(C.c_ubyte)), trav.ctypes.data_as(dp),
                                                      st.ctypes.data_as(C.POINTER(C.c_int)), C.byref(stats)))
        out = (safe[:n].astype(bool), trav[:n], st[:n])
        if want_stats:
            out += ({"n_visits": stats.n_visits, "n_discs": stats.n_discs, "n_radius_classes": stats.n_radius_classes},)
        return out

    def polygon_untraversable_hull(self, polygon, map_index=0, cap=4096):
        """isTraversable(polygon, computeUntraversablePolygon=True): (is_traversable, traversability, hull (k, 2))."""
        v = np.ascontiguousarray(polygon, dtype=np.float64).reshape(-1, 2)
        ok, val, nh = C.c_ubyte(), C.c_double(), C.c_int()
        hull = np.zeros((max(cap, 1), 2), np.float64)
        dp = C.POINTER(C.c_double)
        _check(load().te_polygon_untraversable_hull(self._h, int(map_index), len(v), v.ctypes.data_as(dp), C.byref(ok),
                                                    C.byref(val), int(cap), C.byref(nh), hull.ctypes.data_as(dp)))
        return bool(ok.value), val.value, hull[:nh.value].copy()

    def set_check_robot_inclination(self, enabled):
        """footprint/check_robot_inclination: the path checks then run checkInclination on the layer robot_slope."""
        _check(load().te_set_check_robot_inclination(self._h, int(bool(enabled))))

    def check_inclination(self, segments, map_index=0):
        """Batched TraversabilityMap::checkInclination: segments (n, 4) = start x y, end x y -> (ok[bool], status)."""
        seg = np.ascontiguousarray(segments, dtype=np.float64).reshape(-1, 4)
        n = len(seg)
        ok = np.zeros(max(n, 1), np.uint8)
        st = np.zeros(max(n, 1), np.int32)
        _check(load().te_check_inclination(self._h, int(map_index), n, seg.ctypes.data_as(C.POINTER(C.c_double)),
                                           ok.ctypes.data_as(C.POINTER(C.c_ubyte)), st.ctypes.data_as(C.POINTER(C.c_int))))
        return ok[:n].astype(bool), st[:n]

    def upload_msg(self, msg, layer_name="elevation", layer="elevation"):
        """fromMessage + upload: geometry from the message, layer `layer_name` into device layer `layer`."""
        info = TeMsgInfo()
        _check(load().te_upload_msg(self._h, msg, len(msg), layer_name.encode(),
                                    self._lid(layer), C.byref(info)))
        self.rows, self.cols, self.batch = info.rows, info.cols, 1
        return info

    def upload_image(self, array, encoding=None, lower=0.0, upper=1.0, alpha_threshold=0.5, layer="elevation", map_index=0):
        """addLayerFromImage on the device: an H x W or H x W x C array of uint8 / uint16 (host byte order) into `layer`.
        The array's own row stride is the image's step when its pixels are packed within a row; the encoding defaults from
        dtype and channel count and only decides the layout (the grey value takes the channels in memory order)."""
        a = _image_array(array)
        ch = 1 if a.ndim == 2 else a.shape[2]
        if encoding is not None and IMAGE_ENCODINGS.get(encoding) != (ch, a.itemsize):
            raise ValueError(f"encoding {encoding!r} does not describe {ch} channels of {a.itemsize} bytes")
        packed = a.strides[1:] == ((ch * a.itemsize, a.itemsize) if a.ndim == 3 else (a.itemsize,))
        if not packed or a.strides[0] < a.shape[1] * ch * a.itemsize or a.strides[0] >= 2 ** 31 or a.shape[0] == 1:
            a = np.ascontiguousarray(a)
        info = TeImageInfo(height=a.shape[0], width=a.shape[1], step=a.strides[0], channels=ch, bytes_per_channel=a.itemsize,
                           is_bigendian=1 if sys.byteorder == "big" else 0)
        _check(load().te_upload_image(self._h, C.byref(info), C.c_void_p(a.ctypes.data),
                                      self._lid(layer), int(map_index), float(lower),
                                      float(upper), float(alpha_threshold)))

    def upload_image_msg(self, msg, resolution, position=(0.0, 0.0), lower=0.0, upper=1.0, alpha_threshold=0.5, layer="elevation"):
        """imageCallback: the geometry from the image's size, `resolution` and `position`, its pixels into `layer`."""
        info = TeImageInfo()
        _check(load().te_upload_image_msg(self._h, msg, len(msg), self._lid(layer),
                                          float(lower), float(upper), float(alpha_threshold), float(resolution),
                                          float(position[0]), float(position[1]), C.byref(info)))
        self.rows, self.cols, self.batch = info.height, info.width, 1
        return info

    def download_msg(self, info, layers, basic_layers=()):
        """toMessage: {message layer name: device layer} of map 0 -> serialised grid_map_msgs/GridMap bytes."""
        names = list(layers)
        ids = (C.c_int * max(len(names), 1))(*[self._lid(v) for v in layers.values()])
        need = C.c_size_t()
        L = load()
        args = (self._h, C.byref(info), len(names), ids, _names(names), len(basic_layers), _names(list(basic_layers)))
        L.te_download_msg(*args, None, 0, C.byref(need))
        out = C.create_string_buffer(max(need.value, 1))
        _check(L.te_download_msg(*args, out, need.value, C.byref(need)))
        return out.raw[:need.value]

    def download_occupancy(self, layers, data_min=1.0, data_max=0.0, map_index=0, out=None):
        """toOccupancyGrid on the device: `layers` (names or ids) of one map -> int8 [len(layers), rows * cols], each layer in
        the message's (reversed) cell order.  data_min / data_max: one value or one per layer.  out: a reusable (possibly
        pinned) int8 buffer."""
        ids, n = _layer_ids(layers, self)
        mn = np.ascontiguousarray(np.broadcast_to(np.asarray(data_min, np.float32), (n,)))
        mx = np.ascontiguousarray(np.broadcast_to(np.asarray(data_max, np.float32), (n,)))
        if out is None:
            out = np.empty((n, self.rows * self.cols), np.int8)
        assert out.dtype == np.int8 and out.flags.c_contiguous and out.size == n * self.rows * self.cols
        fpt = C.POINTER(C.c_float)
        _check(load().te_download_occupancy(self._h, int(map_index), n, ids, mn.ctypes.data_as(fpt), mx.ctypes.data_as(fpt),
                                            C.c_void_p(out.ctypes.data)))
        return out

    def download_occupancy_msg(self, info, layer, data_min=1.0, data_max=0.0):
        """toOccupancyGrid of `layer` of map 0 -> serialised nav_msgs/OccupancyGrid bytes (seq, stamp, frame_id from `info`)."""
        need = C.c_size_t()
        L = load()
        args = (self._h, C.byref(info), self._lid(layer), float(data_min), float(data_max))
        L.te_download_occupancy_msg(*args, None, 0, C.byref(need))
        out = C.create_string_buffer(max(need.value, 1))
        _check(L.te_download_occupancy_msg(*args, out, need.value, C.byref(need)))
        return out.raw[:need.value]

    def count_cloud(self, layers, point_layer, basic_layers=(), map_index=0):
        """The sizing call of te_download_cloud: the number of points."""
        ids, n = _layer_ids(layers, self)
        bids, nb = _layer_ids(basic_layers, self)
        cnt = C.c_size_t()
        _check(load().te_download_cloud(self._h, int(map_index), n, ids, _layer_ids([point_layer], self)[0][0], nb, bids, None, 0,
                                        C.byref(cnt)))
        return cnt.value

    def download_cloud(self, layers, point_layer, basic_layers=(), map_index=0, out=None):
        """toPointCloud on the device: float32 [n_points, len(layers) + 2], the point layer's column replaced by x, y, z.
        out: a reusable (possibly pinned) float32 buffer with room for every cell; the result is a view of it."""
        ids, n = _layer_ids(layers, self)
        bids, nb = _layer_ids(basic_layers, self)
        pid = _layer_ids([point_layer], self)[0][0]
        cnt = C.c_size_t()
        L = load()
        if out is None:  # (room for every cell: one call, the count is not run twice)
            out = np.empty(max(self.rows * self.cols, 1) * (n + 2), np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous
        cap = out.size // (n + 2)
        _check(L.te_download_cloud(self._h, int(map_index), n, ids, pid, nb, bids, C.c_void_p(out.ctypes.data), cap, C.byref(cnt)))
        return out.reshape(-1)[:cnt.value * (n + 2)].reshape(cnt.value, n + 2)

    def download_cloud_msg(self, info, layers, point_layer, basic_layers=()):
        """toPointCloud of map 0: {field name: device layer} -> serialised sensor_msgs/PointCloud2 bytes."""
        names = list(layers)
        ids, n = _layer_ids(layers.values(), self)
        bids, nb = _layer_ids(basic_layers, self)
        need = C.c_size_t()
        L = load()
        args = (self._h, C.byref(info), n, ids, _names(names), _layer_ids([point_layer], self)[0][0], nb, bids)
        L.te_download_cloud_msg(*args, None, 0, C.byref(need))
        out = C.create_string_buffer(max(need.value, 1))
        _check(L.te_download_cloud_msg(*args, out, need.value, C.byref(need)))
        return out.raw[:need.value]

    def download_submap(self, position, length, layers, map=0, out=None):
        """GridMap::getSubmap(position, length) of `layers` (names or ids) of one map, packed on the device: returns (info,
        {layer: array[h, w]}) -- views of one float32 buffer --, and (info, {}) when info.ok == 0.  out: a reusable (possibly
        pinned) float32 buffer with room for the submap; without one the geometry call sizes a new buffer."""
        ids, n = _layer_ids(layers, self)
        info = TeSubmapInfo()
        L = load()
        if out is None:
            L.te_download_submap(self._h, int(map), float(position[0]), float(position[1]), float(length[0]), float(length[1]), n, ids,
                                 C.byref(info), None, 0)  # (the sizing call: fills info, or fails as the real one will)
            out = np.empty(max(n * info.rows * info.cols, 1), np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous
        _check(L.te_download_submap(self._h, int(map), float(position[0]), float(position[1]), float(length[0]), float(length[1]), n, ids,
                                    C.byref(info), C.c_void_p(out.ctypes.data), out.size))
        if not info.ok:
            return info, {}
        h, w = info.rows, info.cols
        packed = out.reshape(-1)[:n * w * h].reshape(n, w, h)
        return info, {name: packed[k].T for k, name in enumerate(layers)}

    def download_submap_msg(self, info, position, length, layers, basic_layers=()):
        """toMessage(getSubmap(position, length), layers) of map 0: {message layer name: device layer} -> (TeSubmapInfo,
        serialised grid_map_msgs/GridMap bytes); (info, b"") when the request fails (info.ok == 0).  seq, stamp, frame_id,
        pose z and orientation come from `info` (a TeMsgInfo)."""
        names = list(layers)
        ids, n = _layer_ids(layers.values(), self)
        need = C.c_size_t()
        sub = TeSubmapInfo()
        L = load()
        args = (self._h, C.byref(info), float(position[0]), float(position[1]), float(length[0]), float(length[1]), n, ids, _names(names),
                len(basic_layers), _names(list(basic_layers)), C.byref(sub))
        L.te_download_submap_msg(*args, None, 0, C.byref(need))
        out = C.create_string_buffer(max(need.value, 1))
        _check(L.te_download_submap_msg(*args, out, need.value, C.byref(need)))
        return sub, out.raw[:need.value]

    def run_polygon_footprint(self, points_xy, yaw):
        """traversabilityFootprint(footprintYaw): fills the layers traversability_x / traversability_rot."""
        pts = np.ascontiguousarray(points_xy, dtype=np.float64).reshape(-1, 2)
        _check(load().te_run_polygon_footprint(self._h, len(pts), pts.ctypes.data_as(C.POINTER(C.c_double)), float(yaw)))

    def polygons_traversable(self, polygons, map_index=0):
        """Batched isTraversable(polygon): list of (n_i, 2) vertex arrays -> (traversable bool[n], traversability float64[n])."""
        off, xy = pack_paths(polygons)
        n = len(off) - 1
        ok = np.zeros(max(n, 1), np.uint8)
        trav = np.zeros(max(n, 1), np.float64)
        _check(load().te_polygons_traversable(self._h, int(map_index), n, off.ctypes.data_as(C.POINTER(C.c_int)),
                                              xy.ctypes.data_as(C.POINTER(C.c_double)),
                                              ok.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                              trav.ctypes.data_as(C.POINTER(C.c_double))))
        return ok[:n].astype(bool), trav[:n]

    def check_polygon_footprint_paths(self, paths, points_xyz, conservative=None, map_index=0):
        """Batched checkFootprintPath for a polygonal footprint: paths = list of (n_i, 7) pose arrays (position xyz,
        orientation xyzw); returns (is_safe bool[n], traversability[n], area[n], status[n])."""
        paths = [np.asarray(p, dtype=np.float64).reshape(-1, 7) for p in paths]
        n = len(paths)
        off = np.zeros(n + 1, np.int32)
        if n:
            off[1:] = np.cumsum([len(p) for p in paths])
        poses = np.concatenate(paths) if n and off[-1] else np.zeros((1, 7))
        return self.check_polygon_footprint_paths_packed(off, poses, points_xyz, conservative, map_index)

    def check_polygon_footprint_paths_packed(self, off, poses, points_xyz, conservative=None, map_index=0):
        """The same with the poses already packed: off int32[n+1] (off[0] == 0), poses float64[off[-1], 7]."""
        off = np.ascontiguousarray(off, dtype=np.int32)
        poses = np.ascontiguousarray(poses, dtype=np.float64)
        n = len(off) - 1
        pts = np.ascontiguousarray(points_xyz, dtype=np.float64).reshape(-1, 3)
        cons = None if conservative is None else np.ascontiguousarray(conservative, dtype=np.uint8)
        safe = np.zeros(max(n, 1), np.uint8)
        trav = np.zeros(max(n, 1), np.float64)
        area = np.zeros(max(n, 1), np.float64)
        st = np.zeros(max(n, 1), np.int32)
        dp = C.POINTER(C.c_double)
        _check(load().te_check_polygon_footprint_paths(
            self._h, int(map_index), n, off.ctypes.data_as(C.POINTER(C.c_int)), poses.ctypes.data_as(dp), len(pts),
            pts.ctypes.data_as(dp), None if cons is None else cons.ctypes.data_as(C.POINTER(C.c_ubyte)),
            safe.ctypes.data_as(C.POINTER(C.c_ubyte)), trav.ctypes.data_as(dp), area.ctypes.data_as(dp),
            st.ctypes.data_as(C.POINTER(C.c_int))))
        return safe[:n].astype(bool), trav[:n], area[:n], st[:n]

    def sync(self):
        _check(load().te_sync(self._h))

    def download(self, layer, map0=0, nmaps=None):
        nmaps = self.batch - map0 if nmaps is None else nmaps
        out = np.empty(nmaps * self.rows * self.cols, np.float32)
        _check(load().te_download_layer(self._h, self._lid(layer),
                                        out.ctypes.data_as(C.POINTER(C.c_float)), int(map0), int(nmaps)))
        return out

    def download_into(self, layer, out, map0=0, nmaps=None):
        """te_download_layer into a caller-owned float32 buffer (reused, possibly pinned)."""
        nmaps = self.batch - map0 if nmaps is None else nmaps
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.size == nmaps * self.rows * self.cols
        _check(load().te_download_layer(self._h, self._lid(layer),
                                        out.ctypes.data_as(C.POINTER(C.c_float)), int(map0), int(nmaps)))
        return out

    def time_chain(self, flags=0, warmup=3, iters=10):
        ms = C.c_float()
        _check(load().te_time_chain(self._h, int(flags), int(warmup), int(iters), C.byref(ms)))
        return ms.value

    def time_chain_samples(self, flags=0, warmup=3, iters=100):
        """Device time of each of `iters` launches (HIP events on the context's stream), in ms."""
        ms = (C.c_float * int(iters))()
        _check(load().te_time_chain_samples(self._h, int(flags), int(warmup), int(iters), ms))
        return np.array(ms[:], dtype=np.float64)
