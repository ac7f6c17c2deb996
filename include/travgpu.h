/*
 * travgpu.h -- C-ABI of libtravgpu.so: the MI355X (gfx950) traversability filter chain.
 *
 * This is the drop-in boundary for ONE hot path of leggedrobotics/traversability_estimation: the
 * filter chain that `filter_chain_.update(elevationMapCopy, traversabilityMapCopy)` runs
 * (traversability_estimation/src/TraversabilityMap.cpp:214) plus the circular footprint pass
 * (TraversabilityMap.cpp:307-318).  The shim owns the device-resident elevation and output layers
 * and launches the HIP chain; plain pointers and sizes only, no C++/torch types.
 *
 * Which reference interface each entry point replaces (paths relative to the reference root):
 *
 *   te_set_params        <- FilterBase<T>::getParam() reads in
 *                           traversability_estimation_filters/src/SlopeFilter.cpp:34-56,
 *                           StepFilter.cpp:38-99, RoughnessFilter.cpp:36-70, the
 *                           NormalVectorsFilter / MathExpressionFilter entries of
 *                           traversability_estimation/config/robot_filter_parameter.yaml:3-9,29-33
 *                           and the footprint parameters read in TraversabilityMap.cpp:108-126
 *   te_set_geometry      <- grid_map::GridMap::setGeometry (length/resolution/position) as used by
 *                           TraversabilityMap::setElevationMap, TraversabilityMap.cpp:135-154
 *   te_upload_elevation  <- the "elevation" layer of mapIn handed to every plugin's
 *                           update(const T& mapIn, T& mapOut) (SlopeFilter.cpp:59, StepFilter.cpp:102,
 *                           RoughnessFilter.cpp:73)
 *   te_run_filter        <- one plugin's update(): SlopeFilter.cpp:59-88 / StepFilter.cpp:102-182 /
 *                           RoughnessFilter.cpp:73-132, reading the layers that plugin reads from mapIn
 *   te_run_chain         <- filters::FilterChain<GridMap>::update, TraversabilityMap.cpp:214
 *                           (NormalVectorsFilter -> SlopeFilter::update -> StepFilter::update ->
 *                           RoughnessFilter::update -> MathExpressionFilter -> DeletionFilter)
 *   te_run_footprint     <- TraversabilityMap::traversabilityFootprint(radius, offset),
 *                           TraversabilityMap.cpp:307-318 (isTraversable :654-746,
 *                           isTraversableForFilters :774-792, checkFor{Slope,Step,Roughness} :794-921)
 *   te_download_layer    <- mapOut.add(type_) / mapOut.at(type_, index) results of each plugin
 *                           (SlopeFilter.cpp:63,77-80 etc.)
 *   te_check_footprint_paths, te_check_footprint_paths_radius, te_check_polygon_footprint_paths
 *                        <- TraversabilityMap::checkFootprintPath, TraversabilityMap.cpp:320-342
 *                           (checkCircularFootprintPath :344-462, checkPolygonalFootprintPath :464-584)
 *   te_check_inclination, te_set_check_robot_inclination
 *                        <- TraversabilityMap::checkInclination :748-762 and footprint/check_robot_inclination :114
 *   te_polygons_traversable <- TraversabilityMap::isTraversable(polygon, traversability), :586-645
 *   te_polygon_untraversable_hull <- isTraversable(polygon, computeUntraversablePolygon, ..), :592-645
 *   te_run_polygon_footprint <- TraversabilityMap::traversabilityFootprint(footprintYaw), :239-305
 *   te_upload_msg / te_download_msg / te_msg_* / te_bag_*
 *                        <- GridMapRosConverter::fromMessage / toMessage / loadFromBag / saveToBag as called in
 *                           TraversabilityMap.cpp:135-154 and TraversabilityEstimation.cpp:125-152, 248-270, 318-329
 *   te_image_parse / te_upload_image / te_upload_image_msg
 *                        <- TraversabilityEstimation::imageCallback, TraversabilityEstimation.cpp:154-168
 *                           (GridMapRosConverter::initializeFromImage, then addLayerFromImage(image, "elevation", map,
 *                           min_height, max_height)): the image's own 1 .. 8 bytes per cell cross PCIe, the conversion
 *                           to float32 and the transposition into the column-major layer run on the device
 *   te_download_occupancy / te_download_occupancy_msg / te_download_cloud / te_download_cloud_msg
 *                        <- the grid_map_visualization entries of traversability_estimation/config/visualization/
 *                           traversability.yaml (type occupancy_grid for the four score layers, type point_cloud for the
 *                           elevation): GridMapRosConverter::toOccupancyGrid / toPointCloud, converted on the device
 *   te_submap_geometry / te_download_submap / te_download_submap_msg
 *                        <- the get_traversability service, TraversabilityEstimation.cpp:297-316:
 *                           GridMap::getSubmap(position, length) of the traversability map and toMessage(subMap, layers);
 *                           the rectangle of the requested layers is packed on the device and crosses PCIe in one transfer
 *   te_run_median_fill / te_run_median_fill_region / te_download_fill_mask
 *                        <- gridMapFilters/MedianFillFilter (grid_map_filters; not in the reference tree: restated, see below),
 *                           the hole filling a grid_map pipeline puts in front of the chain
 *   te_run_radius_filter / te_run_radius_filter_region / te_radius_filter_stats
 *                        <- gridMapFilters/MeanInRadiusFilter and MinInRadiusFilter (grid_map_filters; restated, see below):
 *                           the radial blur between the fill and the normals, and the conservative lower surface
 *   te_run_window_expression / te_window_expr_check / te_window_expression_stats
 *                        <- gridMapFilters/SlidingWindowMathExpressionFilter (grid_map_filters; restated, see below): an
 *                           EigenLab expression over a square window around every cell (local deviation, box mean, relief)
 *   te_run_distance / te_run_distance_region / te_distance_stats
 *                        <- no filter of grid_map: the clearance layer a planner asks a traversability map for, the exact
 *                           distance of every cell to the nearest untraversable one (defined below, not restated)
 *   te_run_components / te_run_reachable / te_components_stats
 *                        <- no filter of grid_map: the connected regions of the free cells -- the size of every cell's region,
 *                           and what is connected to the robot (defined below, not restated)
 *
 * Data contract (identical to grid_map::Matrix = Eigen::MatrixXf): float32, COLUMN-major,
 * element (row i, col j) of map m at ptr[m*rows*cols + j*rows + i]; invalid cell = non-finite.
 * The device layers are in logical order; a GridMap that has been move()d (circular-buffer start index != (0,0))
 * goes through te_upload_layer_circular / te_download_layer_circular / te_upload_msg, which rotate inside the copy.
 *
 * All functions return TE_OK (0) or a negative te_status; te_last_error() gives the message of the
 * calling thread's last failure.  A context is internally serialised (one mutex, one HIP stream);
 * different contexts may be used concurrently from different threads.
 */
#ifndef TRAVGPU_H
#define TRAVGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TE_ABI_VERSION 1

typedef enum te_status {
  TE_OK = 0,
  TE_ERR_INVALID_ARG = -1, /* NULL pointer, bad enum, bad size */
  TE_ERR_BAD_PARAM = -2,   /* a filter parameter outside the range the reference's configure() accepts */
  TE_ERR_NOT_READY = -3,   /* geometry/params/elevation missing, or chain not run before footprint */
  TE_ERR_HIP = -4,         /* HIP runtime error (message has hipGetErrorString) */
  TE_ERR_NO_DEVICE = -5,   /* no usable gfx950 device: the library never falls back to the CPU */
  TE_ERR_UNSUPPORTED = -6  /* a filter disc above 32 cells or with more than 32 offsets on its circle, under TE_OPT_FILTER_ANY_RADIUS = 0 (the
                              default); under 1 or 2, and for a circular footprint, only tables that do not fit in device memory; te_expr_check /
                              te_run_expression: valid EigenLab that is not built (the matrix product, transpose, plain min / max ...) */
} te_status;

/* Layers owned by a context (device-resident, [batch][cols][rows] float32). */
typedef enum te_layer {
  TE_LAYER_ELEVATION = 0,
  TE_LAYER_SLOPE = 1,       /* traversability_slope      (SlopeFilter map_type)     */
  TE_LAYER_STEP = 2,        /* traversability_step       (StepFilter map_type)      */
  TE_LAYER_ROUGHNESS = 3,   /* traversability_roughness  (RoughnessFilter map_type) */
  TE_LAYER_TRAVERSABILITY = 4,
  TE_LAYER_FOOTPRINT = 5,   /* traversability_footprint  */
  TE_LAYER_NORMAL_X = 6,    /* surface_normal_{x,y,z}: only kept with TE_RUN_KEEP_NORMALS */
  TE_LAYER_NORMAL_Y = 7,
  TE_LAYER_NORMAL_Z = 8,
  TE_LAYER_SLOPE_FOOTPRINT = 9,   /* memo layers of checkForSlope/Step/Roughness (0/1/NaN) */
  TE_LAYER_STEP_FOOTPRINT = 10,
  TE_LAYER_ROUGHNESS_FOOTPRINT = 11,
  TE_LAYER_TRAVERSABILITY_X = 12,   /* traversability_x / traversability_rot: exist after te_run_polygon_footprint */
  TE_LAYER_TRAVERSABILITY_ROT = 13,
  TE_LAYER_ROBOT_SLOPE = 14,   /* input of checkInclination (robotSlopeType_, TraversabilityMap.cpp:47): optional, exists
                                  from its first upload on (te_upload_layer / _circular / te_upload_msg / te_device_ptr) */
  TE_LAYER_COUNT = 15
} te_layer;
/* Beside the 15 layers above a context holds up to TE_MAX_USER_LAYERS float layers under names of the caller's choice
 * (te_add_layer, below): ids TE_LAYER_COUNT .. TE_LAYER_COUNT + TE_MAX_USER_LAYERS - 1, so that every id fits a 32-bit layer
 * mask (te_expr_info).  An id that was never added is refused wherever an out-of-range id is. */
#define TE_MAX_USER_LAYERS 16

/* te_run_chain flags */
#define TE_RUN_KEEP_NORMALS 0x1u /* also write surface_normal_{x,y,z} (i.e. no DeletionFilter) */
#define TE_RUN_FOOTPRINT    0x2u /* run the circular footprint pass right after the chain */
#define TE_RUN_FOOTPRINT_MEMO 0x8u /* with the footprint pass: also write slope_/step_/roughness_footprint (0/1/NaN) */
#define TE_RUN_SEQUENTIAL 0x10u /* one HIP stream only (default: step filter and normals kernel overlap on two streams) */
#define TE_RUN_NORMALS_ONLY 0x20u /* measurement aid: only the normals/slope/roughness kernel (+ its fix-up pass) */
#define TE_RUN_GENERIC_KERNELS 0x4u /* use only the shape-generic kernels (also the path for tie radii); for A/B tests */

/* The reference's plugins one at a time (te_run_filter): what the drop-in adapters of
 * traversabilityFilters/{Slope,Step,Roughness}Filter call, each reading exactly the layers the
 * reference plugin reads from mapIn. */
typedef enum te_filter {
  TE_FILTER_SLOPE = 1,     /* in: surface_normal_z                      out: traversability_slope     (SlopeFilter.cpp:59-88) */
  TE_FILTER_STEP = 2,      /* in: elevation                             out: traversability_step      (StepFilter.cpp:102-182) */
  TE_FILTER_ROUGHNESS = 3, /* in: elevation, surface_normal_{x,y,z}     out: traversability_roughness (RoughnessFilter.cpp:73-132) */
  TE_FILTER_COMBINE = 4,   /* in: the three scores                      out: traversability           (MathExpressionFilter) */
  TE_FILTER_NORMALS = 5    /* in: elevation                             out: surface_normal_{x,y,z}   (NormalVectorsFilter, area method;
                              robot_filter_parameter.yaml:3-9; README.md:173 "Surface Normals Filter") */
} te_filter;

/* Filter parameters: same keys, defaults and validity ranges as the reference's configure()s.
 * POD; `size` must be sizeof(te_params) (ABI check).  This is the blob that is broadcast to the
 * other ranks (RCCL) when the batch is sharded over several GPUs. */
typedef struct te_params {
  uint32_t size;
  uint32_t abi_version;
  /* gridMapFilters/NormalVectorsFilter: radius, normal_vector_positive_axis */
  double normals_radius;
  int32_t normals_axis; /* 0:x 1:y 2:z */
  int32_t _pad0;
  /* traversabilityFilters/SlopeFilter: critical_value in [0, pi/2] */
  double slope_critical;
  /* traversabilityFilters/StepFilter: critical_value>=0, first/second_window_radius>=0, critical_cell_number>0 */
  double step_critical;
  double step_radius1;
  double step_radius2;
  int32_t step_ncrit;
  int32_t _pad1;
  /* traversabilityFilters/RoughnessFilter: critical_value>=0, estimation_radius>=0 */
  double rough_critical;
  double rough_radius;
  /* gridMapFilters/MathExpressionFilter, fixed form, float32:
   *   traversability = w_scale * ((w_slope*slope + w_step*step) + w_rough*roughness)
   * default (1.0f/3.0f) and 1,1,1 == the shipped expression bit for bit */
  float w_scale, w_slope, w_step, w_rough;
  /* circular footprint: radiusMin = fp_radius, radiusMax = fp_radius + fp_offset */
  double fp_radius;
  double fp_offset;
  double fp_default;       /* footprint/traversability_default */
  double fp_max_gap;       /* max_gap_width */
  double fp_critical_step; /* criticalStepHeight_ = stepFilter.critical_value */
  int32_t fp_check_roughness;
  int32_t _pad2;
} te_params;

typedef struct te_ctx te_ctx;

/* Fill `p` with the shipped defaults (robot_filter_parameter.yaml, robot_footprint_parameter.yaml, robot.yaml). */
int te_params_default(te_params* p);
/* Range checks of the reference's configure()s; TE_ERR_BAD_PARAM + message on violation. */
int te_params_validate(const te_params* p);

int te_device_count(int* count);
int te_create(int device, te_ctx** out);
int te_destroy(te_ctx* ctx);

int te_set_params(te_ctx* ctx, const te_params* p);
int te_get_params(te_ctx* ctx, te_params* p);
/* Choices between kernels that produce IDENTICAL layers (no reference counterpart: the reference has one code path).
 * The defaults pick by input size; the options exist so that tests and measurements can reach every path through the
 * ABI -- the library never reads the environment. */
#define TE_OPT_FP_BLOCKED_WALK 1          /* discs with an untraversable cell: 0 by list length, 1 one disc per wavefront, 2 one disc per lane */
#define TE_OPT_FP_BLOCKED_BLOCKS_PER_CU 2 /* grid of that kernel: 0 default (24), 1 .. 32 */
#define TE_OPT_GRAPH_REPLAY 4             /* whole-map launches as a captured hipGraph: 0 by size (the default: from 2^22 cells), 1 always, 2 never */
#define TE_OPT_POLYGON_PER_CELL 3         /* polygon footprint layers: 1 evaluates every cell of every bounding box instead of the offset table */
#define TE_OPT_BCAST_RCCL 5               /* te_bcast_params, set on the ROOT context: 0 RCCL only between different devices (the default), 1 also when all contexts share one device (a communicator of one rank) */
#define TE_OPT_FP_ANY_REACH 7             /* circular footprint pass: 0 (default) by reach -- up to 20 cells the shape-specialised sum kernels, above 20, and at any reach for a traversability layer without a known bound (te_run_footprint), the route of any reach; 1 the route of any reach for every footprint */
#define TE_OPT_NORMALS_RANK_RULE 6        /* 1: NormalVectorsFilter as grid_map <= 1.6 had it (the filter that wrote TE/maps/elevation_map.bag): a disc whose scatter matrix is rank-deficient -- exactly planar -- gets UnitZ; runs the shape-generic kernels.  0 (default): the current area method */
/* Filter discs (normals, roughness, step windows) of any radius, per context:
 *   0 (default) a disc above 32 cells, or with more than 32 offsets on its circle, is refused with TE_ERR_UNSUPPORTED;
 *   1 any radius: the discs the shape kernels hold keep their routes bit for bit, larger ones take te_filter_any.hip;
 *   2 that route for every filter disc (tests and A/B timing).
 * Takes effect at once when parameters and geometry are held (the discs are rebuilt); if they cannot be -- going back to 0
 * while a 40-cell radius is held -- TE_ERR_UNSUPPORTED, and the option and the discs stay as they were.  te_bcast_params
 * carries parameters only: each receiving context needs the option set as well.  The C++ plugins set 1. */
#define TE_OPT_FILTER_ANY_RADIUS 8
/* Face flags: a whole-layer elevation upload also records, per 64 x 4 cells, whether a drop of more than fp_critical_step
 * between adjacent cells lies within 2 cells; the mask kernel of the footprint pass skips its step-check staging on tiles
 * without one.  1 (default): the flags are passed whenever they are known (they are not after tile uploads, te_device_ptr
 * of the elevation, a failed prefetch, or a te_set_params that changed fp_critical_step -- until the next whole upload);
 * 0: never.  The layers are identical either way. */
#define TE_OPT_FACE_FLAGS 9
/* te_run_median_fill: 0 (default) the kernel the plan names (csrc/te_median_plan.h: the tile kernel while the window radius is
 * at most 15 cells, the general kernel above), 1 the tile kernel wherever its window fits, 2 the general kernel always.  The
 * layers are identical either way, bit for bit. */
#define TE_OPT_MEDIAN_ROUTE 10
/* te_run_radius_filter: 0 (default) the kernel the plan names (csrc/te_radius_plan.h), 1 the sliding kernel wherever its
 * result is provably exact (its segments fit in LDS; a workgroup of the Mean whose values fail the plan's predicate still runs
 * the in-order gather), 2 the in-order gather always.  The layers are identical under every value, bit for bit. */
#define TE_OPT_RADIUS_ROUTE 11
/* te_run_window_expression: 0 (default) the route the plan names (csrc/te_window_plan.h), 1 the separable route wherever it is
 * allowed (no nested reduction, its column partials fit in LDS; a workgroup that `mean` padding gives a clipped window still
 * walks directly), 2 the direct walk always.  The layers are identical under every value, bit for bit. */
#define TE_OPT_WINDOW_EXPR_ROUTE 12
/* gridMapFilters/NormalVectorsFilter `algorithm`: 0 (default) the area method (the PCA plane fit over the disc of normals_radius),
 * 1 the raster method: the normal from the finite differences of a cell's four neighbours (k_normals_raster,
 * csrc/te_normals_raster.hip).  Any other value: TE_ERR_INVALID_ARG.  Unlike the options above this one CHANGES the layers: setting
 * it drops the chain's results and the kept normals (te_ctx_state.h: normals_algorithm_set) and the captured launches.
 *
 * The raster contract (restated, not pinned: grid_map_filters is not in the reference tree; written from memory of the filter
 * shipped with ROS Noetic grid_map 1.6.x).  z: the input layer (float32), element (i, j) of a rows x cols
 * map; res: the resolution (double); x grows towards smaller i, y towards smaller j; finite means isfinite.
 *   1. The outermost line of cells is never visited: all three outputs are NaN where i == 0, i == rows-1, j == 0 or j == cols-1.
 *      A map with fewer than 3 rows or columns is therefore all NaN.
 *   2. An interior cell takes c = z[i,j], t = z[i-1,j], b = z[i+1,j], l = z[i,j-1], r = z[i,j+1], each widened to double.
 *      x direction: gx = (b - t) / (2.0 * res) when t and b are finite; otherwise, when c is finite, gx = (c - t) / res if only t is
 *      finite and gx = (b - c) / res if only b is finite; otherwise none.  y direction: gy likewise with l in place of t and r in
 *      place of b.  If either direction has none, the three outputs are NaN.  An invalid centre between two finite pairs does get
 *      a normal.
 *   3. n = (gx, gy, 1.0); norm = sqrt((gx*gx + gy*gy) + 1.0); every component is divided by norm (a division, not a reciprocal
 *      multiply); every operation is a separately rounded double; n = -n if the component on normal_vector_positive_axis is
 *      < 0.0; the result is stored as float32.  This is (-dz/dx, -dz/dy, 1) normalised.
 * The device's normals are held bit for bit against tests/ref_py/raster_normals_ref.py (tests/test_gpu_raster_normals.py).
 *
 * Under raster:
 *   te_run_filter(TE_FILTER_NORMALS) writes the three normal layers and nothing else; the state afterwards is as after the area
 *     method.
 *   te_run_chain (any batch, every TE_RUN_* flag): the raster kernel writes the normals and traversability_slope (SlopeFilter's
 *     rule on the float32 surface_normal_z), RoughnessFilter runs on those normals by the route TE_FILTER_ROUGHNESS takes (an
 *     invalid centre with a normal gets a roughness, RoughnessFilter.cpp:84), the step filter and the combine as under area.  The
 *     normal layers are written by every run, and count as present afterwards only with TE_RUN_KEEP_NORMALS, as under area.
 *     TE_RUN_NORMALS_ONLY writes the normals and nothing else.
 *   normals_radius is still validated by te_set_params (and its disc is still built: above 32 cells it needs
 *     TE_OPT_FILTER_ANY_RADIUS as under area) but takes no part in results or routing; TE_OPT_NORMALS_RANK_RULE has no effect.
 *   te_run_chain_region returns TE_ERR_UNSUPPORTED: the roughness route on given normals is whole-map only, and a region form of
 *     it is not built. */
#define TE_OPT_NORMALS_ALGORITHM 13
/* te_run_distance: 0 (default) the route of pass 2 the plan names (csrc/te_distance_plan.h), 1 the tiled route wherever its
 * tile fits in LDS, 2 the route of any reach always.  The layers are identical under every value, bit for bit. */
#define TE_OPT_DISTANCE_ROUTE 14
int te_set_option(te_ctx* ctx, int option, int value);
/* The face flags a footprint run would be given now (tests, diagnostics): batch x ceil(cols / 4) x ceil(rows / 64) bytes, the
 * flag of 64 cells along the rows fastest; `bytes` must be exactly that.  TE_ERR_NOT_READY while they are unknown or
 * switched off. */
int te_download_face_flags(te_ctx* ctx, unsigned char* out, size_t bytes);
/* rows = size(0), cols = size(1) of every map of the batch; (pos_x,pos_y) = map centre. */
int te_set_geometry(te_ctx* ctx, int rows, int cols, int batch, double resolution, double pos_x, double pos_y);

/* Host -> device copy of `nmaps` maps starting at batch slot `map0` (column-major float32). */
int te_upload_elevation(te_ctx* ctx, const float* host, int map0, int nmaps);
/* Overwrite the h x w sub-rectangle with top-left cell (row0, col0) of map `map` from a packed
 * column-major h x w host tile (dirty-region update). */
int te_upload_tile(te_ctx* ctx, const float* host_tile, int map, int row0, int col0, int h, int w);
/* Device pointer of a layer ([batch][cols][rows] float32) for zero-copy producers/consumers
 * (e.g. a torch tensor filled on the same device); valid until te_set_geometry/te_destroy.
 * Writers order their work against the context themselves (te_sync, or the same device stream order).  Handing out
 * TE_LAYER_TRAVERSABILITY marks that layer as caller-writable until the next te_set_geometry: te_run_footprint and
 * region runs then no longer assume its values are bounded by the chain's weights (they sum it on the route of any
 * reach, see te_run_footprint); te_run_chain with TE_RUN_FOOTPRINT rewrites every cell first and is unaffected. */
int te_device_ptr(te_ctx* ctx, int layer, void** dptr, size_t* bytes);
/* The optional input layer robot_slope (checkInclination, TraversabilityMap.cpp:748-762; it travels with the elevation
 * map when the caller has one) is present after an upload.  present = 0 declares it absent again -- an elevation map that
 * comes without the layer must not be checked against the previous map's -- and present = 1 declares a buffer filled
 * through te_device_ptr ready.  With check_robot_inclination set the path checks fail (TE_ERR_NOT_READY) while the
 * layer is absent, like the reference's atPosition() throws for a missing layer. */
int te_set_layer_present(te_ctx* ctx, int layer, int present);

/* Host -> device copy of any layer (e.g. surface_normal_z for TE_FILTER_SLOPE); elevation marks the context ready. */
int te_upload_layer(te_ctx* ctx, int layer, const float* host, int map0, int nmaps);
/* te_upload_tile for any layer that has memory: the same packed column-major h x w tile, the same checks.  TE_LAYER_ELEVATION
 * IS te_upload_tile (the done-flags stay, counts and face flags are unknown until the next whole upload); any other layer is
 * afterwards what te_upload_layer of the patched values leaves.  Synchronous.  With it unfiltered elevation tiles go into a
 * holding layer, in front of te_run_median_fill_region / te_run_radius_filter_region. */
int te_upload_layer_tile(te_ctx* ctx, int layer, const float* host_tile, int map, int row0, int col0, int h, int w);
/* The same for a layer in GridMap's circular-buffer order: logical cell (i, j) is stored at ((i + start_row) % rows,
 * (j + start_col) % cols) (grid_map_core getBufferIndexFromIndex; start index = GridMap::getStartIndex(), non-zero after
 * GridMap::move).  The reference's filters see maps in this form: their iterators (StepFilter.cpp:112,124) hide the
 * start index.  The device layers are always in logical order. */
int te_upload_layer_circular(te_ctx* ctx, int layer, const float* host, int map, int start_row, int start_col);
int te_download_layer_circular(te_ctx* ctx, int layer, float* host, int map, int start_row, int start_col);
/* Whole-layer uploads (all maps of the batch) that run BESIDE the calls that follow: the reference's FilterChain hands every
 * plugin the whole map (SlopeFilter.cpp:62-63, StepFilter.cpp:105-107, RoughnessFilter.cpp:76-77), so a plugin knows which
 * layers its successors will read (StepFilter: elevation; RoughnessFilter: elevation + surface_normal_{x,y,z}) and can send
 * them host -> device while its own filter runs and its output crosses device -> host -- PCIe is full duplex.  Returns at
 * once; a thread of the library stages the buffers through a second ring of page-locked slots.  Until te_wait_prefetch
 * returns the host buffers must stay valid.  te_run_filter, te_download_layer(_circular), te_get_params / te_set_params
 * run BESIDE a prefetch in flight as long as they neither read nor write one of its layers; a call that does (e.g.
 * TE_FILTER_STEP beside an elevation prefetch, a download of a prefetched layer) and every other entry point finish the
 * prefetch first -- no call ever sees a half-written layer.  A prefetch that failed leaves its layers undefined:
 * te_wait_prefetch reports it, and an elevation layer among them must be uploaded again before the next chain
 * (TE_ERR_NOT_READY until then).  A prefetched elevation layer is scanned for invalid cells when the prefetch is joined (one
 * short kernel on the context's stream and a wait for its two counters, as te_upload_elevation does): the count and the
 * run count pick the normals kernel's march and strip height (hole-free, scattered cells, unobserved regions).  n <= 8. */
int te_prefetch_layers(te_ctx* ctx, int n, const int* layers, const float* const* hosts);
int te_wait_prefetch(te_ctx* ctx);
/* Run ONE of the reference's plugins on the resident layers (see te_filter). */
int te_run_filter(te_ctx* ctx, int filter, unsigned flags);
int te_run_chain(te_ctx* ctx, unsigned flags);
/* Re-filter only the cells whose outputs can change when the h x w rectangle at (row0,col0) of map
 * `map` changed (the rectangle dilated by the chain's reach). */
/* With TE_RUN_FOOTPRINT (| TE_RUN_FOOTPRINT_MEMO) the circular footprint pass follows on the cells that can see the
 * change (the re-filtered cells grown by 3 cells for isTraversableForFilters and by the footprint's reach); the
 * traversability_footprint layer must have been complete before (te_run_chain with the flag, or te_run_footprint),
 * TE_ERR_NOT_READY otherwise.  The caller of the reference's node re-filters the whole map on every update
 * (TraversabilityMap.cpp:202-237); this is the incremental form of the same call.
 * A footprint shape none of the shape-specialised sum kernels takes (a tie radius that is not a whole number of cells,
 * a reach of 17..20 cells, a map narrower than 64 cells) is served by the general kernel, which recomputes the footprint
 * layer of the WHOLE map `map` (no other map of the batch): cost O(map), not O(region); cells outside the region are
 * recomputed from unchanged inputs and keep their values to within the fixed-point kernels' rounding (< 1e-6).
 * A reach above 20 cells, TE_OPT_FP_ANY_REACH = 1, or a traversability layer without a known bound (te_run_footprint):
 * the route of any reach recomputes the column prefix sums of the whole map `map` (one streaming pass over its 5 bytes
 * per cell, writing 12) and the footprint on the region grown by the reach only. */
int te_run_chain_region(te_ctx* ctx, unsigned flags, int map, int row0, int col0, int h, int w);
/* The h x w rectangle at (row0, col0) of a layer of map `map` into a packed column-major h x w host tile (the layout
 * te_upload_tile reads); returns when the tile is in host memory. */
int te_download_tile(te_ctx* ctx, int layer, int map, int row0, int col0, int h, int w, float* host_tile);
/* Streaming updates (BASELINE configs[4]: a resident map, one dirty tile per tick).  te_upload_tile_async returns at
 * once: the tile crosses PCIe on the context's copy-in stream into a device staging slot -- concurrently with the kernels
 * of the previous tick -- and is placed into the elevation layer on the compute stream, in order with the launches
 * that follow (te_run_chain_region).  te_download_tile_async is its mirror: the rectangle is copied to a staging slot in
 * order with the launches before it and crosses PCIe on the copy-out stream while the next tick computes.  Two slots
 * each way.  host_tile must stay valid until te_sync (which waits for all three streams) -- page-lock it (te_pin_host),
 * otherwise the runtime stages the copy itself and the call blocks for its duration. */
int te_upload_tile_async(te_ctx* ctx, const float* host_tile, int map, int row0, int col0, int h, int w);
int te_download_tile_async(te_ctx* ctx, int layer, int map, int row0, int col0, int h, int w, float* host_tile);
/* The circular footprint pass over the resident layers (te_run_chain with TE_RUN_FOOTPRINT runs the same pass).
 * Values of the traversability layer: the chain's own layer under weights w with w_scale * (w_slope + w_step + w_rough)
 * and |fp_default| small enough -- the reference's weights are -- is summed by the shape-specialised kernels (fixed point
 * within 1e-6 of the reference, or in double).  Every other layer -- written by te_upload_layer, te_run_expression or
 * through te_device_ptr, combined per plugin, or combined with a negative weight, a large weight or beside a large
 * fp_default -- has no known bound and is summed on the route of any reach: untraversable cells are counted in integers,
 * exactly, whatever the values are, and the values of either sign are summed in double as differences of one running
 * prefix sum per map column.  The error of a disc's sum is therefore NOT local to the disc: it is of the order of
 * (2 * reach + 1) * 2^-52 * A, with A the sum of |values| (fp_default for non-finite ones, as in the reference) over the
 * WHOLE column of the map (worst case: 7 roundings of 2^-53 * A more per 64 rows), and the mean carries that divided by
 * the disc's cells plus float32 rounding.
 * Supported and tested: |values| up to 1e6 on maps of a few thousand rows, held to 1e-5 * max(1, max |value| of the layer)
 * (tests/test_gpu_footprint_values.py), and a magnitude ratio of 1e6 within one column, held to (2 * reach + 1) * 2^-48 * A on 96 rows.  Beyond
 * that nothing is detected and no error is returned; precision degrades gradually by the same formula: a disc of small
 * values in a column that also holds values 1e10 times larger loses about 1e-5 of its mean, and at a ratio of 2^52 (one
 * cell of 1e20 above cells of 1) the small values vanish from the sums altogether.  Layers of such dynamic range must be
 * rescaled or clamped by the caller.  That route takes 12 bytes of device memory per cell, allocated when such a layer is
 * first summed (TE_ERR_UNSUPPORTED if they do not fit). */
int te_run_footprint(te_ctx* ctx);
/* Batched TraversabilityMap::checkFootprintPath for circular footprints (TraversabilityMap.cpp:320-342 ->
 * checkCircularFootprintPath :344-462) on the resident traversability_footprint layer of map `map`, which must be
 * complete (te_run_chain with TE_RUN_FOOTPRINT or te_run_footprint, with fp_radius = the paths' radius and
 * fp_offset = 0.15 like :348): isTraversable() then takes its memo branch (:672-677) for every centre.
 * Path k has the poses pose_xy[2*pose_offset[k] .. 2*pose_offset[k+1]) (x, y in the map frame; pose_offset[0] == 0).
 * Outputs per path: is_safe and traversability (TraversabilityResult, :352-355), status 0 ok / 1 a pose of a
 * multi-pose path lies outside the map (the reference ignores getIndex()'s failure there: undefined) / 2 no poses
 * (:330-334).  With te_set_check_robot_inclination(ctx, 1) every pose of a one-pose path / every segment first passes
 * checkInclination (:366-370, :390-394) on the layer robot_slope; a failure leaves the default result (unsafe, 0), and
 * status 1 also marks a position checkInclination was handed outside the map (atPosition throws there).  Reference
 * options not covered: publishPolygons (ROS markers) and the untraversable polygon of compute_untraversable_polygon, which
 * on a complete footprint layer is Polygon::fromCircle of the unsafe centres (:676-678) -- no map data; the result is
 * the same with and without it.  Host buffers; synchronous. */
int te_check_footprint_paths(te_ctx* ctx, int map, int n_paths, const int* pose_offset, const double* pose_xy,
                             unsigned char* is_safe, double* traversability, int* status);
/* The same check with every path at its OWN radius (FootprintPath.radius, TraversabilityMap.cpp:347-348) and without a
 * footprint layer: the value at a visited centre is isTraversable(centre, radius[k] + offset, radius[k]) evaluated on demand
 * (:681-735 with computeUntraversablePolygon = false, the radiusMin == 0 branch and the static_cast<float> of the memo store
 * included), at the centres the paths visit and nowhere else -- what the reference does on the all-NaN footprint layer
 * computeTraversability leaves behind.  A request that mixes k radii costs one call, not k whole-map footprint passes.
 *   precondition: the chain has run on the map (te_run_chain / te_run_chain_region): TE_ERR_NOT_READY otherwise.  The
 *     footprint pass need not have run; TE_LAYER_FOOTPRINT is neither read nor written, and the call changes neither the
 *     three memo layers nor the parameters te_get_params returns.
 *   radius[n_paths], offset (0.15 in the reference, :348): negative or non-finite values give TE_ERR_INVALID_ARG for the
 *     whole call.  At most 65536 distinct radii per call.
 *   outputs, status codes, check_robot_inclination, traversabilityDefault_ (fp_default) for a centre outside the map, the
 *     nSkip = 3 walk and the length-weighted mean: those of te_check_footprint_paths.
 *   memo: lives for this one call, keyed by (centre cell, radius, offset).  The reference keeps ONE memo layer for all
 *     radii, so there a value computed for one radius answers a later query at another radius; that accident of its state
 *     is deliberately not reproduced.  The reference also stops a path at its first unsafe centre; the batch evaluates
 *     every visited centre, the results are the same.
 *   stats (may be NULL): n_visits centres visited by all paths (a one-pose path outside the map visits none; a path stops
 *     at a segment with an end outside the map), n_discs distinct (cell, radius) discs evaluated, n_radius_classes
 *     distinct radii.
 * The untraversable-cell mask the discs read does not depend on the radius: it is built on the first call after the
 * scores changed and kept until they, fp_max_gap, fp_critical_step or fp_check_roughness change.  Scratch memory follows
 * the number of visits, not the map.  Not covered: publishPolygons, and the untraversable polygon of the on-demand branch
 * (the convex hull at :729).  Host buffers; synchronous. */
typedef struct te_path_check_stats {
  int n_visits, n_discs, n_radius_classes;
} te_path_check_stats;
int te_check_footprint_paths_radius(te_ctx* ctx, int map, int n_paths, const int* pose_offset, const double* pose_xy,
                                    const double* radius, double offset, unsigned char* is_safe, double* traversability,
                                    int* status, te_path_check_stats* stats);
/* footprint/check_robot_inclination (TraversabilityMap.cpp:114, default false): when set, te_check_footprint_paths and
 * te_check_polygon_footprint_paths run checkInclination before every isTraversable, reading TE_LAYER_ROBOT_SLOPE (the
 * reference's layer "robot_slope", written by whoever estimates the robot's inclination); TE_ERR_NOT_READY from the
 * path checks if that layer was never uploaded. */
int te_set_check_robot_inclination(te_ctx* ctx, int enabled);
/* Batched TraversabilityMap::checkInclination(start, end) (:748-762) on the layer robot_slope of map `map`: segment k =
 * start_end_xy[4k .. 4k+4) = start x y, end x y.  start == end: ok = the cell's value != 0; otherwise a LineIterator from
 * the start index to the end index, cells that are not valid skipped, ok = no cell is 0.  status 0 / 1 a position lies
 * outside the map (ok = 0 then).  Host buffers; synchronous. */
int te_check_inclination(te_ctx* ctx, int map, int n_segments, const double* start_end_xy, unsigned char* ok, int* status);
/* TraversabilityMap::traversabilityFootprint(footprintYaw) (TraversabilityMap.cpp:239-305): for every cell of every map the
 * footprint polygon (n_points vertices points_xy = x0 y0 x1 y1 .. in the footprint frame, footprint/footprint_polygon
 * :91-103) centred on the cell, as given -> layer traversability_x, and turned by `yaw` about z -> traversability_rot;
 * each cell gets isTraversable(polygon)'s mean (:586-645) or 0 when the polygon touches an untraversable cell.  Needs a
 * footprint pass over the resident chain (te_run_chain with TE_RUN_FOOTPRINT or te_run_footprint first; TE_ERR_NOT_READY
 * otherwise).  The untraversable-cell mask that pass leaves behind is what the kernels read; where a score layer was
 * written since (te_upload_layer, a prefetch, te_device_ptr), after te_move_map with results kept, or after a region run
 * that found the mask not done, the call builds the mask again from the scores now resident before it reads it -- as
 * te_check_footprint_paths_radius does, and as the reference, which evaluates isTraversableForFilters on the live score
 * layers.  At most TE_MAX_POLYGON_VERTICES points.  Asynchronous like te_run_chain; read the layers
 * with te_download_layer(TE_LAYER_TRAVERSABILITY_X / _ROT). */
#define TE_MAX_POLYGON_VERTICES 32
int te_run_polygon_footprint(te_ctx* ctx, int n_points, const double* points_xy, double yaw);
/* Batched TraversabilityMap::isTraversable(polygon, traversability) (:586-645) on map `map`: polygon k has the vertices
 * vertex_xy[2*vertex_offset[k] .. 2*vertex_offset[k+1]) in the map frame (at least one each; vertex_offset[0] == 0).
 * traversability[k] = mean over the polygon's cells, traversabilityDefault_ when it covers no cell centre, 0 when
 * is_traversable[k] == 0.  The per-segment polygons of checkPolygonalFootprintPath (:464-584) go through this.  Same
 * precondition, and the same rule for a mask that is not done, as above.  Host buffers; synchronous. */
int te_polygons_traversable(te_ctx* ctx, int map, int n_polygons, const int* vertex_offset, const double* vertex_xy,
                            unsigned char* is_traversable, double* traversability);
/* TraversabilityMap::isTraversable(polygon, computeUntraversablePolygon = true, traversability, untraversablePolygon)
 * (:592-645; FootprintPath.compute_untraversable_polygon) for ONE polygon on map `map`: is_traversable / traversability as
 * te_polygons_traversable, plus the untraversable polygon = grid_map::Polygon::monotoneChainConvexHullOfPoints of the
 * positions of every untraversable cell inside the polygon (*n_hull = 0 when traversable; the points as collected when
 * there are at most three).  hull_xy holds cap_vertices vertices (x y); TE_ERR_INVALID_ARG with *n_hull set if the hull
 * has more.  The device reduces every row of the bounding box to its outermost untraversable cells, the chain runs on
 * the host.  For circular footprints on a complete footprint layer the reference's untraversable polygon is just
 * Polygon::fromCircle(center, radius + offset) of an unsafe centre (:676-678): no map data, left to the caller.
 * Same precondition as te_polygons_traversable.  Host buffers; synchronous. */
int te_polygon_untraversable_hull(te_ctx* ctx, int map, int n_vertices, const double* vertex_xy, unsigned char* is_traversable,
                                  double* traversability, int cap_vertices, int* n_hull, double* hull_xy);
/* Batched TraversabilityMap::checkFootprintPath for polygonal footprints (checkPolygonalFootprintPath, :464-584).
 * Path k has the poses poses[7*pose_offset[k] .. 7*pose_offset[k+1]) -- position x y z, orientation x y z w, as in
 * geometry_msgs/Pose; the footprint is n_points points x y z (path.footprint.polygon.points) in the footprint frame;
 * conservative[k] = path.conservative (NULL: all false).  The pose polygons (toPosition * orientation * point), their
 * conservative extensions, the convex hull of consecutive ones (grid_map::Polygon::convexHull) and the areas are computed
 * on the host, every polygon's isTraversable on the device in one launch.  Outputs per path = TraversabilityResult:
 * is_safe, traversability, area (a path that fails keeps the values of the segments before, as the reference's result
 * does).  status: 0 ok, 1 check_robot_inclination is set and a position handed to checkInclination lies outside the map,
 * 2 no poses (:330-334), 3 the conservative vertex lists outgrew 1024 vertices.  With te_set_check_robot_inclination
 * checkInclination runs before every polygon (:526-528, :553-557).  Not covered: publishPolygons (ROS markers); the
 * untraversable polygon of compute_untraversable_polygon is te_polygon_untraversable_hull on the polygons
 * te_path_polygons returns (it is only ever published, :531-533, :559-561; the result is the same).  Host buffers; synchronous. */
int te_check_polygon_footprint_paths(te_ctx* ctx, int map, int n_paths, const int* pose_offset, const double* poses, int n_points,
                                     const double* points_xyz, const unsigned char* conservative, unsigned char* is_safe,
                                     double* traversability, double* area, int* status);
/* Host part of the above on its own (no device, no context): the polygons checkPolygonalFootprintPath hands to
 * isTraversable -- the pose polygon of a one-pose path, the convex hull of consecutive (conservatively extended) pose
 * polygons otherwise -- e.g. to publish them like publishFootprintPolygon (:527, :558).  Path k owns the polygons
 * polygon_first[k] .. polygon_first[k+1]); polygon p has the vertices vertex_xy[2*vertex_offset[p] .. 2*vertex_offset[p+1])
 * and the area area[p] (Polygon::getArea).  *n_polygons / *n_vertices receive the totals; nothing is written beyond
 * cap_polygons polygons / cap_vertices vertices (TE_ERR_INVALID_ARG then: call once with zero capacities to size).
 * Poses and footprint points must be finite (TE_ERR_INVALID_ARG).  The per-path status of the full check is not reported
 * here: a path without poses owns no polygon (polygon_first[k] == polygon_first[k+1]); a path whose conservative vertex
 * lists outgrow 1024 vertices ends with the last polygon that fits (te_check_polygon_footprint_paths reports status 3). */
int te_path_polygons(int n_paths, const int* pose_offset, const double* poses, int n_points, const double* points_xyz,
                     const unsigned char* conservative, int cap_polygons, int cap_vertices, int* n_polygons, int* n_vertices,
                     int* polygon_first, int* vertex_offset, double* vertex_xy, double* area);
int te_sync(te_ctx* ctx);

int te_download_layer(te_ctx* ctx, int layer, float* host, int map0, int nmaps);
/* Page-lock a host buffer the caller keeps across frames (a GridMap layer that lives as long as the node): uploads from
 * and downloads into it then run as direct DMA instead of through the runtime's staging copies.  te_unpin_host before
 * the buffer is freed.  Purely an optimisation: every transfer entry point accepts pageable memory too. */
int te_pin_host(void* host, size_t bytes);
int te_unpin_host(void* host);

/* ---- several GPUs from one process -------------------------------------------------------------
 * The path shards on the batch axis only: maps are independent, there is no data-path collective.  A host that owns
 * all GPUs of a node (the reference's node is one process) creates one context per device, gives every context its
 * block of the batch, and drives them from one thread -- every entry point above is asynchronous on its context's own
 * stream, so the devices run side by side.
 *   te_shard_range      contiguous block [first, first + count) of `batch` maps owned by shard k of n (sizes differ by
 *                       at most one map; the same split as traversability_estimation_amd/dist.py)
 *   te_bcast_params     every context receives the parameters of ctxs[root].  Contexts on different devices get the
 *                       te_params block through an RCCL broadcast over xGMI (librccl is loaded when first needed;
 *                       communicators are created per call: this is configure-time, TraversabilityMap.cpp:764-772);
 *                       contexts sharing the root's device are copied on the host.  TE_ERR_UNSUPPORTED if several
 *                       devices are involved and librccl cannot be loaded.
 *   te_run_chain_multi  te_run_chain(flags) on every context, in order, without waiting
 *   te_sync_multi       te_sync on every context */
int te_shard_range(int batch, int n_shards, int k, int* first, int* count);
int te_bcast_params(te_ctx** ctxs, int n, int root);
int te_run_chain_multi(te_ctx** ctxs, int n, unsigned flags);
int te_sync_multi(te_ctx** ctxs, int n);

/* Time `iters` back-to-back te_run_chain(flags) launches with HIP events on the context's stream
 * (after `warmup` untimed ones); inputs and outputs stay resident in HBM. */
int te_time_chain(te_ctx* ctx, unsigned flags, int warmup, int iters, float* ms_per_iter);
/* The same, one event pair per launch: ms[k] = device time of the k-th launch (for a median; the launches are not
 * back to back, every one is waited for). */
int te_time_chain_samples(te_ctx* ctx, unsigned flags, int warmup, int iters, float* ms);

/* ---- wire formats either side of the chain: grid_map_msgs/GridMap (ROS1 serialisation) and rosbag V2.0 ----
 * The reference node gets its elevation map as such a message (TraversabilityEstimation.cpp:248-270 requestElevationMap ->
 * GridMapRosConverter::fromMessage), loads / saves maps from / to bags (:125-152 loadFromBag, :318-329 saveToBag) and
 * publishes its result with toMessage.  A layer's float32 payload in the message IS the layer's Eigen matrix
 * (column-major, circular start index = outer/inner_start_index), so it moves between the message buffer and the device
 * with te_upload_layer_circular's rectangle copies: no host-side GridMap, no reshuffling. */
#define TE_MSG_MAX_NAME 64
typedef struct te_msg_info {
  uint32_t seq, stamp_sec, stamp_nsec; /* info.header */
  char frame_id[TE_MSG_MAX_NAME];      /* NUL-terminated */
  double resolution, length_x, length_y;
  double pose[7];                /* position x y z, orientation x y z w; GridMap uses position x, y only */
  int32_t rows, cols;            /* size of every layer: dim[1].size, dim[0].size */
  int32_t start_row, start_col;  /* outer_start_index, inner_start_index = GridMap::getStartIndex()(0), (1) */
  int32_t n_layers, n_basic_layers;
} te_msg_info;

/* Validate a serialised message and describe it.  Rejected (TE_ERR_INVALID_ARG + message): truncation, layers/data count
 * mismatch (fromMessage's own check), storage order other than (column_index, row_index), layer sizes that disagree with
 * each other or with round(length / resolution), start index outside the map. */
int te_msg_parse(const void* msg, size_t len, te_msg_info* info);
/* Name of layer k (NUL-terminated into name[TE_MSG_MAX_NAME]) and byte offset of its rows*cols float32 payload. */
int te_msg_layer(const void* msg, size_t len, int k, char* name, size_t* data_offset);
/* toMessage for host layers: layer_data[k] = rows*cols float32 in the GridMap's own (column-major, circular) storage order;
 * every field of `info` is used.  *written = bytes needed even when `cap` is too small (out = NULL, cap = 0 sizes). */
int te_msg_write(const te_msg_info* info, int n_layers, const char* const* names, const float* const* layer_data, int n_basic,
                 const char* const* basic_names, void* out, size_t cap, size_t* written);
/* fromMessage + upload in one step: (re)sets the context's geometry from the message (batch 1: rows, cols, resolution,
 * position) when it differs, then copies layer `layer_name` into device layer `layer` (te_layer), undoing the circular
 * start index.  `info` (may be NULL) receives the parsed description. */
int te_upload_msg(te_ctx* ctx, const void* msg, size_t len, const char* layer_name, int layer, te_msg_info* info);
/* toMessage: serialise n_layers device layers (te_layer ids `layers`, message names `names`) of map 0 into `out`.
 * Geometry comes from the context; seq, stamp, frame_id, pose z / orientation and the start index from `info` (its
 * rows / cols / lengths / resolution are ignored).  *written = bytes needed even when TE_ERR_INVALID_ARG reports that
 * `cap` is too small (call with out = NULL, cap = 0 to size the buffer). */
int te_download_msg(te_ctx* ctx, const te_msg_info* info, int n_layers, const int* layers, const char* const* names, int n_basic,
                    const char* const* basic_names, void* out, size_t cap, size_t* written);
/* loadFromBag: the last grid_map_msgs/GridMap message stored under `topic` in an (uncompressed-chunk) rosbag V2.0 image. */
int te_bag_find_message(const void* bag, size_t len, const char* topic, size_t* msg_offset, size_t* msg_len);
/* saveToBag: a one-message bag (stamp 0.0 is written as ros::TIME_MIN like the reference).  Sizing call as above. */
int te_bag_write(const void* msg, size_t msg_len, const char* topic, uint32_t stamp_sec, uint32_t stamp_nsec, void* out,
                 size_t cap, size_t* written);

/* ---- sensor_msgs/Image as an input: the reference's image_elevation topic (TraversabilityEstimation.cpp:154-168) ----
 * Accepted encodings (those of grid_map_ros's switch on the cv type): mono8 / 8UC1, mono16 / 16UC1, rgb8 / bgr8 / 8UC3,
 * rgba8 / bgra8 / 8UC4, rgb16 / bgr16 / 16UC3, rgba16 / bgra16 / 16UC4.
 *
 * Semantics = GridMapCvConverter::addLayerFromImage<Type, N> (restated here: grid_map is not vendored):
 *   - Cell (row i, col j) of the layer takes image pixel (row i, column j).  The layer ends up in logical order, start
 *     index 0.  T is uint8 or uint16.  16-bit samples are byte-swapped when is_bigendian differs from the host.
 *   - maxv = (float)numeric_limits<T>::max().
 *   - thr = (T)(alpha_threshold * maxv), truncated.  This gives 127 or 32767 at the default 0.5.
 *   - With 4 channels, a pixel whose last channel is < thr leaves the cell NaN.  (The reference's add(layer) fills NaN
 *     first.)
 *   - Otherwise the float32 operations below run without contraction (the build's -ffp-contract=off):
 *         v = lower + (upper - lower) * ((float)g / maxv)
 *   - g is the sample itself for 1 channel.
 *   - For 3 or 4 channels it is the integer grey value
 *         g = (c0*3735 + c1*19235 + c2*9798 + 16384) >> 15
 *     c0, c1, c2 are the first three channels IN MEMORY ORDER, WHATEVER THE ENCODING SAYS: grid_map calls
 *     cvtColor(..., BGR2GRAY) for rgb and bgr alike.  That quirk is reproduced.
 * The three weights and the shift are OpenCV 4's fixed-point BGR2GRAY as remembered.  Neither OpenCV nor grid_map is part
 * of this project's build, so the colour branch has no reference-held vector (like the footprint half):
 * the formula above is a stated contract that nothing here can pin.  The mono and alpha branches have no such doubt.
 *
 * Rejected with TE_ERR_INVALID_ARG and a message: any other encoding, a truncated message, step below the row's bytes, a
 * data length other than step * height, sizes whose product overflows, a NULL pointer, alpha_threshold outside [0, 1],
 * non-finite lower or upper, and a geometry that is set but whose rows or cols differ from height or width
 * (addLayerFromImage's "Image size does not correspond to grid map size").  te_upload_image without a geometry:
 * TE_ERR_NOT_READY.
 *
 * After an image went into TE_LAYER_ELEVATION the context is exactly what te_upload_elevation of the same floats leaves
 * (invalid cells counted -- alpha holes are holes --, elevation present, chain / footprint / mask results dropped); any
 * other layer follows te_upload_layer.  Both upload calls are synchronous: the host buffer is free on return. */
typedef struct te_image_info {
  uint32_t seq, stamp_sec, stamp_nsec; /* header */
  char frame_id[TE_MSG_MAX_NAME];      /* NUL-terminated */
  int32_t height, width, step;         /* step = bytes per image row, >= width * channels * bytes_per_channel */
  int32_t channels, bytes_per_channel; /* 1|3|4, 1|2 */
  int32_t is_bigendian;
  char encoding[TE_MSG_MAX_NAME];
} te_image_info;

/* ROS1 serialisation of sensor_msgs/Image: header, height, width, encoding, is_bigendian, step, data[].  *data_offset =
 * byte offset of the step * height pixel bytes inside the message. */
int te_image_parse(const void* msg, size_t len, te_image_info* info, size_t* data_offset);
/* addLayerFromImage: pixels (height x width, row pitch `step`, any alignment) -> layer `layer` of map `map`.  Reads only
 * height, width, step, channels, bytes_per_channel and is_bigendian of `info`: a caller with a raw buffer fills those six. */
int te_upload_image(te_ctx* ctx, const te_image_info* info, const void* pixels, int layer, int map, float lower, float upper,
                    double alpha_threshold);
/* imageCallback in one step: parse, (re)set the geometry like initializeFromImage when it differs (batch 1, rows = height,
 * cols = width, resolution, position), then te_upload_image into map 0.  `info` (may be NULL) receives the description. */
int te_upload_image_msg(te_ctx* ctx, const void* msg, size_t len, int layer, float lower, float upper, double alpha_threshold,
                        double resolution, double pos_x, double pos_y, te_image_info* info);

/* ---- nav_msgs/OccupancyGrid as an output: what traversability_estimation/config/visualization/traversability.yaml asks
 * for (traversability, traversability_slope, traversability_step, traversability_roughness, each with data_min 1.0 and
 * data_max 0.0) and what a costmap-based planner consumes.  One byte per cell crosses PCIe instead of four.
 *
 * Semantics = GridMapRosConverter::toOccupancyGrid(gridMap, layer, dataMin, dataMax, grid) (restated here: grid_map_ros is
 * not vendored, so like the image route's colour branch this is a stated contract with no reference-held vector, DESIGN.md
 * section 7).  For every cell, in float32, in this order, without contraction, with a correctly rounded division:
 *       v    = (layer(i, j) - data_min) / (data_max - data_min)
 *       cell = isnan(v) ? -1 : (int8)(0.0f + min(max(0.0f, v), 1.0f) * 100.0f)          (the conversion truncates)
 *       data[n - 1 - (j * rows + i)] = cell                                              n = rows * cols
 *   - +-inf clamp to 0 or 100.  data_min == data_max gives inf or NaN by the formula (0, 100 or -1); it is not rejected.
 *   - The output is the layer's storage order reversed: grid_map's "reverse cell order" of
 *     getLinearIndexFromIndex(.., rowMajor = false).  Device layers have start index (0, 0): nothing to unwrap.
 *   - info.resolution = (float)resolution, info.width = rows, info.height = cols,
 *     info.origin.position = (pos_x - len_x / 2, pos_y - len_y / 2, 0), info.origin.orientation = (0, 0, 0, 1),
 *     info.map_load_time = the header stamp.
 * Wire layout (ROS1, little endian): Header{u32 seq; u32 sec; u32 nsec; string frame_id}
 *   MapMetaData{u32 sec; u32 nsec; f32 resolution; u32 width; u32 height; f64[7] origin}  int8[] data (u32 length, bytes).
 *
 * The calls read the layers and change nothing in the context: chain results, present flags and parameters stay. */
typedef struct te_occupancy_info {
  uint32_t seq, stamp_sec, stamp_nsec;   /* header */
  char frame_id[TE_MSG_MAX_NAME];        /* NUL-terminated */
  uint32_t map_load_sec, map_load_nsec;  /* info.map_load_time */
  float resolution;
  uint32_t width, height;                /* rows, cols of the layer */
  double origin[7];                      /* position x y z, orientation x y z w */
} te_occupancy_info;

/* n_layers (1 .. 16) layers of map `map` -> out[k * rows * cols ..), layer k with its own data_min[k] / data_max[k]: ONE
 * launch and ONE device -> host transfer of n_layers * rows * cols bytes, whatever n_layers is.  `out` may be pageable or
 * page-locked (te_pin_host).  Synchronous.  TE_ERR_NOT_READY: no geometry, or a layer that does not exist (yet);
 * TE_ERR_INVALID_ARG: NULL, a layer id or map index out of range, n_layers out of range, non-finite data_min / data_max. */
#define TE_OCCUPANCY_MAX_LAYERS 16
int te_download_occupancy(te_ctx* ctx, int map, int n_layers, const int* layers, const float* data_min, const float* data_max,
                          int8_t* out);
/* toOccupancyGrid of layer `layer` of map 0 as a serialised message; the cells land directly at their offset in `out`.
 * seq, stamp and frame_id come from `info`, everything else from the context.  *written = bytes needed even when
 * TE_ERR_INVALID_ARG reports that `cap` is too small (out = NULL, cap = 0 sizes the buffer without touching the device). */
int te_download_occupancy_msg(te_ctx* ctx, const te_msg_info* info, int layer, float data_min, float data_max, void* out,
                              size_t cap, size_t* written);
/* Host only, no context: the message of `info` with the width * height cells `data`.  Sizing call as above. */
int te_occupancy_msg_write(const te_occupancy_info* info, const int8_t* data, void* out, size_t cap, size_t* written);
/* Validate and describe a serialised nav_msgs/OccupancyGrid; *data_offset = byte offset of its width * height cells.
 * Rejected (TE_ERR_INVALID_ARG + message): truncation, a frame_id longer than TE_MSG_MAX_NAME - 1, width * height other
 * than the data length, a product that overflows. */
int te_occupancy_parse(const void* msg, size_t len, te_occupancy_info* info, size_t* data_offset);

/* ---- sensor_msgs/PointCloud2 as an output: the visualization config's point cloud of the elevation layer.  Only the valid
 * cells cross PCIe.
 *
 * Semantics = GridMapRosConverter::toPointCloud(gridMap, layers, pointLayer, cloud) (restated, as above):
 *   - The point layer must appear in `layers` exactly once.  A point's record is the layers in order, one float32 field
 *     each, named after the layer; the point layer is replaced by the three fields x, y, z.  n_fields = n_layers + 2,
 *     point_step = 4 * n_fields, offsets 0, 4, 8, ..., datatype 7 (FLOAT32), count 1.
 *   - x, y = (float) of the cell centre's double position (x(i) = pos_x + (len_x / 2 - res / 2) + res * (double)(-i), y(j)
 *     likewise), z = the point layer's value, every other field = that layer's value (NaN included).
 *   - A cell is emitted iff its point-layer value is finite and, with a basic-layer list, every basic layer is finite there
 *     (GridMap::isValid(index, basicLayers)).
 *   - Points come in GridMapIterator order; with start index (0, 0) that is storage order j * rows + i.
 *   - height = 1, width = n_points, row_step = width * point_step, is_bigendian = 0, is_dense = 0.
 *   - Not covered: the colour special case (a layer named "color" becoming the field "rgb"); the context owns no such layer.
 * Wire layout: Header, u32 height, u32 width, PointField[]{string name; u32 offset; u8 datatype; u32 count}, u8 is_bigendian,
 *   u32 point_step, u32 row_step, u8[] data, u8 is_dense.
 *
 * The compaction keeps the order with three launches on the context's stream -- per-workgroup counts, an exclusive scan of
 * the counts, a scatter -- and no workgroup ever waits for another inside a kernel.  The count comes back with one small
 * synchronous copy before the payload.  Scratch memory follows the map size; it is allocated on first use and kept. */
#define TE_CLOUD_MAX_LAYERS 16
typedef struct te_cloud_info {
  uint32_t seq, stamp_sec, stamp_nsec; /* header */
  char frame_id[TE_MSG_MAX_NAME];      /* NUL-terminated */
  uint32_t height, width;
  uint32_t n_fields, point_step, row_step;
  int32_t is_bigendian, is_dense;
} te_cloud_info;

/* layers[n_layers] (1 .. TE_CLOUD_MAX_LAYERS te_layer ids, point_layer among them exactly once) of map `map`; basic_layers
 * [n_basic] (may be 0 / NULL).  out receives n_points records of n_layers + 2 floats.  *n_points is always set when the
 * count succeeded; more points than cap_points: TE_ERR_INVALID_ARG and nothing is written (cap_points = 0, out = NULL sizes).
 * Error codes as te_download_occupancy.  Synchronous; the context is left as it was. */
int te_download_cloud(te_ctx* ctx, int map, int n_layers, const int* layers, int point_layer, int n_basic, const int* basic_layers,
                      float* out, size_t cap_points, size_t* n_points);
/* toPointCloud of map 0 as a serialised message: field names[k] for layer k (the point layer's name is not used: x, y, z),
 * seq / stamp / frame_id from `info`.  Sizing call as te_download_msg (it runs the count). */
int te_download_cloud_msg(te_ctx* ctx, const te_msg_info* info, int n_layers, const int* layers, const char* const* names,
                          int point_layer, int n_basic, const int* basic_layers, void* out, size_t cap, size_t* written);
/* Host only: a cloud of info->width points (height 1) with n_fields float32 fields named field_names[k], offsets 4k; reads
 * seq, stamp, frame_id, width, is_dense of `info`.  points = width * n_fields floats. */
int te_cloud_msg_write(const te_cloud_info* info, int n_fields, const char* const* field_names, const float* points, void* out,
                       size_t cap, size_t* written);
/* Validate and describe a serialised sensor_msgs/PointCloud2; *data_offset = byte offset of its row_step * height bytes.
 * Rejected: truncation, a name longer than TE_MSG_MAX_NAME - 1, a field datatype outside 1 .. 8 or a field that ends behind
 * point_step, width * point_step above row_step, row_step * height other than the data length, a product that overflows. */
int te_cloud_parse(const void* msg, size_t len, te_cloud_info* info, size_t* data_offset);
/* Field k of a valid message: name (NUL-terminated into name[TE_MSG_MAX_NAME]), offset, datatype, count. */
int te_cloud_field(const void* msg, size_t len, int k, char* name, uint32_t* offset, uint32_t* datatype, uint32_t* count);
/* The spans of the compaction (tests place holes across them): cells[0] = cells of one wavefront's ballot, cells[1] = cells
 * one workgroup counts, cells[2] = cells one scan workgroup's span covers. */
int te_cloud_spans(size_t cells[3]);

/* ---- submap requests: the data path behind the get_traversability service (TraversabilityEstimation.cpp:297-316) ----
 * A planner names a position, a length and a list of layers; the node answers with GridMap::getSubmap(position, length) of the
 * traversability map, serialised by toMessage(subMap, layers).  Only the rectangle of the named layers crosses PCIe.
 *
 * Semantics = GridMap::getSubmap / getSubmapInformation (RESTATED here: grid_map_core is not in the reference tree, so like the
 * image and output routes this is a stated contract with no reference-held vector) for a map whose start
 * index is (0, 0), which device layers always have.  IEEE double, grid_map's order of operations, per axis (len = cells * res):
 *   - corner = position +- length / 2, bounded to the map by boundPositionToRange:
 *         shifted = (corner - map_position) + len / 2;  eps = 10 * DBL_EPSILON, times |corner| when |corner| > 1
 *         shifted <= 0 -> eps;  shifted >= len -> len - eps;  bounded = (shifted + map_position) - len / 2
 *   - index = (int)(-(((bounded - len / 2) - map_position) / res)), truncated; row0 / col0 from the corner at + length / 2, the
 *     last row / column from the one at - length / 2.  rows = last - first + 1, likewise cols.
 *   - the submap's length = rows * res (cols * res); its position = ((map_position + (len / 2 - res / 2)) + res * (double)(-first)
 *     + res / 2) - length / 2.
 *   - ok = 0 (getSubmap returns false; the service answers isSuccess = false) when a bounded corner is still outside the map
 *     (checkIfPositionWithinMap: -((p - map_position) - len / 2) in [0, len)), when the first index is no cell of the map, or
 *     when the requested position lies outside the submap's own geometry -- a centre outside the map, for one.
 *   - a request larger than the map is clamped to it; length 0 gives the one cell under the bounded corners.
 * Arguments are checked first: a non-finite position or length, a negative length (and, in te_submap_geometry, rows or cols
 * below 1, a resolution that is not positive and finite, a non-finite map position) give TE_ERR_INVALID_ARG. */
typedef struct te_submap_info {
  int32_t ok, row0, col0, rows, cols;          /* the rectangle in the map; everything but `ok` is 0 when ok == 0 */
  double pos_x, pos_y, length_x, length_y;     /* the submap's own geometry */
} te_submap_info;
/* Host only, no context: the geometry of one request on a rows x cols map at (pos_x, pos_y). */
int te_submap_geometry(int rows, int cols, double resolution, double pos_x, double pos_y, double req_x, double req_y,
                       double req_len_x, double req_len_y, te_submap_info* out);
/* The submap of n_layers (1 .. 16; an id may repeat) layers of map `map`: out[(k * cols + j) * rows + i] = layer k at
 * (row0 + i, col0 + j), rows / cols / row0 / col0 those of *info -- the column-major submap matrices one after another, which
 * is the payload toMessage carries for them.  ONE launch and ONE device -> host transfer, whatever n_layers is; `out` may be
 * pageable or page-locked (te_pin_host).  Synchronous.
 *   *info is filled whenever the arguments pass their checks.  info->ok == 0: TE_OK, nothing is written.
 *   cap_floats below n_layers * rows * cols: TE_ERR_INVALID_ARG, *info filled (size the buffer from it), nothing is written.
 *   TE_ERR_NOT_READY: no geometry; TE_ERR_INVALID_ARG: NULL, a layer id that is out of range or names a layer that does not
 *   exist yet (as te_download_msg), a map index or n_layers out of range, the request checks above.
 * A prefetch in flight on one of the layers is joined first.  The call reads the layers and changes nothing in the context:
 * chain, footprint and mask results, present flags and parameters stay. */
#define TE_SUBMAP_MAX_LAYERS 16
int te_download_submap(te_ctx* ctx, int map, double req_x, double req_y, double req_len_x, double req_len_y, int n_layers,
                       const int* layers, te_submap_info* info, float* out, size_t cap_floats);
/* toMessage(subMap, layers) of map 0 as a serialised grid_map_msgs/GridMap, through the writer behind te_msg_write: resolution,
 * lengths and position (pose x, y) are the submap's own, the start index is (0, 0); seq, stamp, frame_id, pose z and
 * orientation come from `info_in` (its other fields are ignored); layer k is named names[k].  The packed cells land in `out`
 * with one transfer and the header is written behind them: a call that fails on the device leaves no valid-looking message.
 * *written = bytes needed even when TE_ERR_INVALID_ARG reports that `cap` is too small (out = NULL, cap = 0 sizes the buffer
 * without touching the device); info->ok == 0: TE_OK, *written = 0, nothing is written. */
int te_download_submap_msg(te_ctx* ctx, const te_msg_info* info_in, double req_x, double req_y, double req_len_x,
                           double req_len_y, int n_layers, const int* layers, const char* const* names, int n_basic,
                           const char* const* basic_names, te_submap_info* info, void* out, size_t cap, size_t* written);

/* ---- moving a resident map: GridMap::move for the device layers ----
 * elevation_mapping's map is robot-centric: it move()s whenever the robot has crossed a cell.  te_move_map shifts what the
 * context holds instead of dropping it (te_set_geometry to a new position drops every result and the caller uploads the
 * whole map again).  Device layers stay in logical order; there is no start index.
 *
 * Semantics = GridMap::move's index shift (RESTATED from memory of grid_map_core, not pinned: DESIGN.md section 7), per axis:
 *     s = (requested - held) / resolution;  shift = (int)(s + 0.5 * sign(s))      (halves round away from zero; |s| is
 *     clamped to 2^30 cells before the cast);  new position = held + shift * resolution -- the ALIGNED shift, not the request.
 *   A map moved by +k cells in x holds its old cell i at i + k (x(i) = ax - resolution * i); likewise y and the columns.
 *   A zero shift on both axes changes nothing, not even the position (n_rects = 0, results_kept = 1).
 *   A shift of at least the map's extent on an axis exposes every cell (all_exposed = 1, one rectangle: the map).
 * rects: up to four rectangles (row0, col0, h, w), in this order, each present only where it applies:
 *   1. exposed (rect_exposed = 1): the full-width band of rows whose source lies outside the old window;
 *   2. exposed: the band of such columns, without the rows of 1. -- no cell is in both;
 *   3. trailing line (rect_exposed = 0): on a row shift, the one-row line of the map along the border OPPOSITE to band 1;
 *   4. trailing line: on a column shift, the one-column line along the border opposite to band 2.
 *   The exposed cells hold NaN (0 in the stored fill mask) until the caller uploads them.  The trailing lines carry no new
 *   data, but cells near them were interior before the move: their filter discs and footprints reached cells that have
 *   left the map, and the reference clips every iterator to the map, so their results are stale.  te_run_chain_region on the
 *   line re-filters exactly the cells within reach of that border.  Lines may cross each other and touch the exposed bands.
 * results_kept (CAVEAT 1, tie radii): a cell exactly on a disc's circle is decided from the rounded double positions of the
 *   cells, centre by centre, so results computed at the old position can differ from results at the new one by a whole step.
 *   If one of the five discs of the parameters (normals, roughness, both step windows, footprint radius + offset) has cells
 *   on its circle -- the classification of te_disc.h that routes the kernels, erring towards "tie" -- or no parameters are
 *   set, or TE_OPT_NORMALS_ALGORITHM = 1 (region runs are refused there), results_kept = 0: the layers are still shifted and
 *   the inputs valid, but the context is as after a whole te_upload_elevation; upload the exposed rectangles and run
 *   te_run_chain.  The move then costs a whole-map run but no whole-map upload.  Otherwise results_kept = 1 (CAVEAT 2, the
 *   trailing lines): the context is as after te_upload_tile -- chain, footprint and present flags stay -- and every
 *   rectangle, trailing lines included, must be handed to te_run_chain_region (an exposed one after its te_upload_tile)
 *   before the results are read; the untraversable mask counts as not built until a whole pass or a path check rebuilds it.
 *   CAVEAT 3, the footprint layer: the footprint checks' own windows, circle(3 res) of checkForSlope / checkForRoughness and
 *   circle(2.5 res) of checkForStep, have cells on their circle at EVERY resolution, so isTraversableForFilters -- and with it
 *   traversability_footprint -- of a few cells depends on the position whatever the parameters (measured on the CPU oracle
 *   alone: 10 of 49 152 cells of a 256 x 192 window moved by (+7, -3) cells).  The four chain layers do not.  A caller that
 *   wants the footprint layer of the new position bit for bit passes the rectangles to te_run_chain_region WITHOUT the
 *   footprint flags and runs te_run_footprint once behind them: a whole-map footprint pass, no whole-map chain and no
 *   whole-map upload (capi's Context.refresh_moved does so).  With the footprint flags on the region
 *   runs the layer is the old position's on those cells.
 * te_move_map moves EVERY layer that has memory (all TE_LAYER_*, borrowed holding layers included, robot_slope and the polygon
 * layers once they exist), every map of the batch (one position), the stored fill mask of te_run_median_fill and the
 * untraversable mask.  Each layer is shifted out of place into a scratch of one layer of one map -- no workgroup reads what
 * another of the same launch writes -- and copied back; the scratch is allocated by the first move that needs it and freed
 * with the layers.  Asynchronous on the context's stream, in order with the launches before and after; a prefetch in flight
 * is joined first.  A captured whole-map launch is dropped (as te_set_geometry with the shape held does) and captured anew.
 *   TE_ERR_NOT_READY: no geometry.  TE_ERR_BAD_PARAM: a position that is not finite.  TE_ERR_UNSUPPORTED, before anything is
 *   written or changed: the scratch does not fit in device memory, or the layers hold 2^31 cells or more (all maps) -- such
 *   maps are REFUSED, not moved (the kernel's index arithmetic is 64-bit all the same).  `info` may be NULL. */
typedef struct te_move_info {
  int32_t shift_rows, shift_cols;   /* cells; old cell (i, j) is now (i + shift_rows, j + shift_cols) */
  int32_t n_rects, results_kept, all_exposed, _pad0;
  double pos_x, pos_y;              /* the position held after the move */
  int32_t rects[4][4];              /* (row0, col0, h, w) */
  int32_t rect_exposed[4];          /* 1: exposed cells (upload them), 0: a trailing line (re-filter only) */
} te_move_info;
/* Host only, no context: the plan of one move of a rows x cols map held at (pos_x, pos_y).  params = NULL: results_kept = 0.
 * (TE_OPT_NORMALS_ALGORITHM is a context option: te_move_map clears results_kept under raster, this call cannot know.)
 * TE_ERR_INVALID_ARG: NULL out, rows or cols below 1, a resolution that is not positive and finite, a held position that is
 * not finite; TE_ERR_BAD_PARAM: a requested position that is not finite. */
int te_move_geometry(int rows, int cols, double resolution, double pos_x, double pos_y, double new_x, double new_y,
                     const te_params* params, te_move_info* out);
int te_move_map(te_ctx* ctx, double new_x, double new_y, te_move_info* info);

/* ---- gridMapFilters/MathExpressionFilter with ANY expression (robot_filter_parameter.yaml:29-33) ----
 * te_run_chain / TE_FILTER_COMBINE run the weighted sum of the three scores (te_params: w_scale, w_slope, w_step, w_rough) and
 * keep their fused path.  te_run_expression evaluates any expression of the language below over the resident layers into
 * TE_LAYER_TRAVERSABILITY, one pass over the map (plus two short reduction launches when the text holds reductions).
 *
 * The language restates EigenLab as MathExpressionFilter uses it on MatrixXf.  EigenLab is not part of the reference tree nor of
 * this project's build, so like the image and output routes this is a STATED CONTRACT restated from memory;
 * the one reference-held pin is the shipped expression on the bag map.
 *   operands   a layer by its reference name (elevation, traversability_slope, traversability_step, traversability_roughness,
 *              traversability, traversability_footprint, surface_normal_x / _y / _z, slope_footprint, step_footprint,
 *              roughness_footprint, traversability_x, traversability_rot, robot_slope); a number (digits with an optional
 *              fraction and exponent, or .digits), read as (float)(double)text.  Every value is float32 and every operation
 *              rounds to float32.  A node is a scalar (1 x 1) or a map; a scalar broadcasts.
 *   operators  + - (binary, any mix of scalar and map); * with at least one scalar side (map * map is EigenLab's MATRIX product:
 *              TE_ERR_UNSUPPORTED, write .* instead); .* ./ and / element-wise (map / map is the element-wise quotient);
 *              ^ with a scalar exponent and .^ are element-wise powf, left-associative; unary - and + bind as in MATLAB:
 *              -a^2 = -(a^2), 2^-1 is allowed; parentheses.
 *   functions  abs sqrt square exp log log10 sin cos tan asin acos, element-wise; cwiseMin(a, b) = (b < a) ? b : a and
 *              cwiseMax(a, b) = (a < b) ? b : a -- std::min / std::max operand order, so they are NOT symmetric in NaN: a NaN in
 *              `a` is returned, a NaN in `b` is dropped.
 *   reductions sum mean sumOfFinites meanOfFinites minOfFinites maxOfFinites numberOfFinites of any element-wise
 *              sub-expression, taken per map of the batch; the result is a scalar.  They do not nest; at most 4 per expression.
 *              Sums accumulate in double in a fixed order (the same bits run after run) and are rounded to float32 at the end;
 *              mean = sum / count in double, then rounded.  A map without a finite cell gives NaN for min / max /
 *              meanOfFinites and 0 for sumOfFinites / numberOfFinites.
 *   constants  folded at compile time through + - * / and unary minus only (exact in IEEE float32 on both sides), never through
 *              a function.
 *   limits     64 instructions after folding, 8 distinct layers, an operand stack of 8, 4 reductions, 64 nested parentheses /
 *              prefix signs.
 *   errors     TE_ERR_BAD_PARAM, the message carries the column: syntax errors, unknown names, wrong arity, a limit above.
 *              TE_ERR_UNSUPPORTED: valid EigenLab that is not built -- the matrix product, transpose, trace, norm, zeros / ones /
 *              eye and the other matrix functions, plain min / max (Eigen's NaN behaviour there depends on its version),
 *              indexing, assignment, relational operators. */
typedef struct te_expr_info {
  int32_t n_instructions; /* after constant folding, reduction arguments included */
  uint32_t layer_mask;    /* bit TE_LAYER_* of every layer the expression reads */
  int32_t n_reductions;
  int32_t stack_depth;    /* deepest operand stack of the main expression and of the reduction arguments */
} te_expr_info;
/* Host only, no context: compiles `text` and describes it (`info` may be NULL). */
int te_expr_check(const char* text, te_expr_info* info);
/* traversability = text, on every map of the batch; asynchronous on the context's stream like te_run_chain.
 *   out_layer must be TE_LAYER_TRAVERSABILITY, the filter's output_layer (TE_ERR_INVALID_ARG otherwise).  The layer may appear
 *     in the text: the evaluation is in place, cell by cell, behind the reductions.
 *   TE_ERR_NOT_READY: no geometry; an input layer that does not exist yet -- surface_normal_* unless the last whole-map chain
 *     ran with TE_RUN_KEEP_NORMALS (or they were uploaded / written by TE_FILTER_NORMALS), the three memo layers before a
 *     footprint pass wrote them, traversability_x / _rot before te_run_polygon_footprint, robot_slope while absent.
 *   A failed call leaves every layer as it was.
 *   Afterwards the context is what te_upload_layer(TE_LAYER_TRAVERSABILITY, the same values) leaves: the layer counts as
 *     written from outside (te_run_footprint takes the route of any reach), footprint and mask results follow the upload
 *     path, the chain's state and te_get_params are untouched.  te_run_footprint and the path checks then read the new values;
 *     the next te_run_chain writes the weighted sum again.
 *   A prefetch in flight that writes a layer the text reads (or the traversability layer) is joined first.
 *   On a dirty rectangle: te_run_expression_region evaluates a text without a reduction on a rectangle of one map, and
 *     te_run_chain_region_expression is te_run_chain_region with the text in the place of the weighted sum -- the whole tick in
 *     one call, the footprint half included (below). */
int te_run_expression(te_ctx* ctx, const char* text, int out_layer);
/* traversability = text on the cells of the rectangle (row0, col0) + (h, w) of map `map`; every other cell of every map is
 * untouched.  The evaluator is the whole-map call's, cell by cell: the cells carry the bits te_run_expression would write now.
 * The reach is 0: a cell's value is read from the same cell of the input layers.
 *   out_layer must be TE_LAYER_TRAVERSABILITY (TE_ERR_INVALID_ARG otherwise, as te_run_expression).
 *   TE_ERR_UNSUPPORTED + message: a text with a reduction -- a map-wide meanOfFinites changes with one cell and then changes
 *     every cell: run te_run_expression --; a text that reads the traversability layer itself -- "what the whole-map call
 *     would write now" is not defined for a rectangle recomputed in place.
 *   TE_ERR_NOT_READY: no geometry, an input layer that does not exist yet (as te_run_expression).  TE_ERR_INVALID_ARG: a bad
 *     map, a rectangle outside the map (as te_run_chain_region).  A failed call leaves every layer as it was.
 *   Afterwards the context is what te_upload_layer_tile(TE_LAYER_TRAVERSABILITY, the rectangle, the same values) leaves: the
 *     layer counts as written from outside, the done-flags stay.  Asynchronous on the context's stream; a prefetch in flight
 *     that writes a layer the text reads (or the traversability layer) is joined first. */
int te_run_expression_region(te_ctx* ctx, const char* text, int out_layer, int map, int row0, int col0, int h, int w);
/* The whole tick in one locked call: exactly te_run_chain_region(flags, map, row0, col0, h, w), except that the combined layer
 * on the rectangle the chain recombines -- the region grown by the chain's reach, clamped to the map -- is `text` by the
 * rules of te_run_expression_region instead of the weighted sum.  The footprint half (TE_RUN_FOOTPRINT[_MEMO]) runs behind it
 * on the same cells as in te_run_chain_region; its precondition (a complete footprint layer) is the same, and it plans without
 * a bound of the combined layer (the route of any reach), the layer being an expression's.
 *   text == NULL: te_run_chain_region.  The refusals of te_run_expression_region (a reduction, a text that reads the
 *   traversability layer: TE_ERR_UNSUPPORTED; a missing input layer: TE_ERR_NOT_READY) are checked before anything is launched.
 *   Refused under TE_OPT_NORMALS_ALGORITHM = 1 like te_run_chain_region; every other error as te_run_chain_region.
 *   Afterwards: what te_run_chain_region(flags, ...) followed by te_upload_layer_tile(TE_LAYER_TRAVERSABILITY) leaves.
 *   Precondition as for the region chain: the combined layer outside that rectangle holds te_run_expression(text) of scores
 *   that have not changed since. */
int te_run_chain_region_expression(te_ctx* ctx, unsigned flags, const char* text, int map, int row0, int col0, int h, int w);
/* Measurement aid: `iters` te_run_expression launches of `text`, one HIP event pair each, ms[k] = device time of the k-th
 * (after `warmup` untimed ones), like te_time_chain_samples.  text = NULL times te_run_filter(TE_FILTER_COMBINE) the same way: the
 * weighted sum's own kernel, the yardstick of tools/expr_bench.py. */
int te_time_expression_samples(te_ctx* ctx, const char* text, int warmup, int iters, float* ms);

/* ---- user layers: a grid_map filter chain under its own layer names ----
 * A chain file is written around layers of its own (elevation_filled, elevation_smooth, slope, edges, ...).  A context holds up
 * to TE_MAX_USER_LAYERS of them beside the reference's 15; none is part of the slab (each is an allocation of its own).
 *   name      matches [A-Za-z_][A-Za-z0-9_]{0,62}, is none of the 15 reference names and no function, reduction or refused
 *             EigenLab function name of the expression language (TE_ERR_BAD_PARAM otherwise).
 *   ids       handed out lowest free first; adding a name that exists returns its id with TE_OK; with all 16 in use
 *             TE_ERR_UNSUPPORTED.
 *   memory    a user layer gets its memory from its first write, as robot_slope does (every cell NaN until written; handing
 *             out te_device_ptr counts as that write), and is present from then on.  Reading an absent one -- a download, an
 *             input of a filter or an operand of an expression -- is TE_ERR_NOT_READY.  te_set_layer_present(layer, 0 / 1)
 *             declares it absent / present again (1 needs memory).  te_set_geometry with another shape drops the contents and
 *             keeps the names; a pointer from te_device_ptr is valid until then or until te_remove_layer.
 *   where     a user id is taken wherever any float layer is: te_upload_layer / _tile / _circular, te_download_layer /
 *             _circular / te_download_tile, te_device_ptr, te_prefetch_layers, te_run_median_fill, te_run_radius_filter,
 *             te_run_window_expression and their region forms, te_download_occupancy / _cloud / _submap, te_upload_msg /
 *             te_download_msg, te_run_layer_expression, te_run_threshold, te_copy_layer.  te_move_map shifts the present ones
 *             with the other layers (exposed cells NaN).
 *   state     writing a user layer changes none of the chain's cached results (te_ctx_state.h: user_layer_written).
 * te_remove_layer is gridMapFilters/DeletionFilter: the memory and the name are freed (a prefetch in flight is joined
 * first); TE_ERR_INVALID_ARG for a reference layer or an id that was never added.
 * te_layer_id knows the reference names too (TE_ERR_INVALID_ARG: no such layer); te_layer_name writes the name with its
 * terminator (TE_ERR_INVALID_ARG: no such layer, or cap too small). */
int te_add_layer(te_ctx* ctx, const char* name, int* layer);
int te_remove_layer(te_ctx* ctx, int layer);
int te_layer_id(te_ctx* ctx, const char* name, int* layer);
int te_layer_name(te_ctx* ctx, int layer, char* out, size_t cap);

/* ---- expressions over any layer ----
 * te_expr_check_ctx is te_expr_check with the context's user names as operands beside the reference's.
 * te_run_layer_expression is te_run_expression into any layer that has memory or gets it from its first write (robot_slope,
 * a user layer); the operands are reference and user names.  The evaluator, its limits and its bits are te_run_expression's.
 *   out_layer == TE_LAYER_TRAVERSABILITY: te_run_expression(_region), bit for bit and state for state.
 *   any other reference layer: afterwards the context is what te_upload_layer(out_layer, the same values) leaves (the region
 *     form: te_upload_layer_tile) -- TE_LAYER_ELEVATION counts as replaced and is counted again.
 *   a user layer: nothing else changes.
 *   In place (out_layer in the text) works on whole maps; the region form refuses it, and a text with a reduction, with
 *     TE_ERR_UNSUPPORTED as te_run_expression_region does.
 *   TE_ERR_INVALID_ARG: out_layer is no layer, or one without memory that a write does not give any (traversability_x / _rot
 *     before te_run_polygon_footprint).  TE_ERR_NOT_READY: no geometry, an operand that does not exist yet. */
int te_expr_check_ctx(te_ctx* ctx, const char* text, te_expr_info* info);
int te_run_layer_expression(te_ctx* ctx, const char* text, int out_layer);
int te_run_layer_expression_region(te_ctx* ctx, const char* text, int out_layer, int map, int row0, int col0, int h, int w);

/* ---- gridMapFilters/ThresholdFilter and DuplicationFilter on the device ----
 * grid_map_filters is not in the reference tree: like the other restated filters this contract is RESTATED from memory, not
 * pinned by a vector the reference holds.  The yardstick of the tests is the same contract in numpy
 * (tests/ref_py/pointwise_ref.py).
 *   te_run_threshold   in place on maps [map0, map0 + nmaps) of `layer`:
 *                        TE_THRESHOLD_LOWER  v < (float)threshold ? (float)set_to : v
 *                        TE_THRESHOLD_UPPER  v > (float)threshold ? (float)set_to : v
 *                      A NaN cell stays NaN (both comparisons are false).  The layer must exist (TE_ERR_NOT_READY otherwise, as an
 *                      input of te_run_median_fill); TE_ERR_INVALID_ARG: a bad layer, mode or map range, a NaN threshold.
 *   te_copy_layer      dst = src on those maps, a copy on the device; dst gets memory if a write gives it any.  src == dst
 *                      is TE_OK and does nothing.
 * Afterwards the context is what te_upload_layer (the region form: te_upload_layer_tile) of the same values into the written
 * layer leaves.  Asynchronous on the context's stream. */
#define TE_THRESHOLD_LOWER 1
#define TE_THRESHOLD_UPPER 2
int te_run_threshold(te_ctx* ctx, int layer, int mode, double threshold, double set_to, int map0, int nmaps);
int te_run_threshold_region(te_ctx* ctx, int layer, int mode, double threshold, double set_to, int map, int row0, int col0, int h, int w);
int te_copy_layer(te_ctx* ctx, int src, int dst, int map0, int nmaps);
/* A chain file typically ends MathExpressionFilter -> ThresholdFilter(lower) -> ThresholdFilter(upper) on one layer: three
 * passes for what one cell decides alone.  This is te_run_layer_expression followed by the n te_run_threshold calls on
 * out_layer (all maps), in ONE launch and with exactly their bits: the thresholds ride behind the expression's code as two
 * internal opcodes (not part of the language) and count against its 64 instructions.
 *   n in 0 .. TE_MAX_FUSED_THRESHOLDS.  TE_ERR_BAD_PARAM: the text with its thresholds no longer fits -- the caller then issues
 *   the calls separately.  Every other refusal and the state afterwards: te_run_layer_expression(_region). */
#define TE_MAX_FUSED_THRESHOLDS 4
typedef struct te_threshold {
  int32_t mode; /* TE_THRESHOLD_LOWER / TE_THRESHOLD_UPPER */
  int32_t _pad;
  double threshold, set_to;
} te_threshold;
int te_run_layer_expression_thresholds(te_ctx* ctx, const char* text, int out_layer, int n, const te_threshold* t);
int te_run_layer_expression_thresholds_region(te_ctx* ctx, const char* text, int out_layer, int n, const te_threshold* t, int map, int row0,
                                              int col0, int h, int w);

/* ---- gridMapFilters/MedianFillFilter on the device: hole filling in front of the chain ----
 * grid_map_filters is neither in the reference tree nor vendored: like the image, occupancy and submap routes this contract is
 * RESTATED from memory of the filter shipped with the ROS Noetic grid_map, and nothing in it is pinned by a vector the
 * reference holds.  The yardstick of the tests is the same contract in numpy (tests/ref_py/median_fill_ref.py).
 *   1. window radius in cells  r = (size_t)(radius / resolution): a double division, truncated, no rounding fix
 *      (0.15 / 0.05 = 2.9999999999999996 gives 2);
 *   2. window                  the square [i - r, i + r] x [j - r, j + r], each bound clamped to the map (not a disc);
 *   3. median(window)          over the FINITE values of the input layer in the window (+-inf is left out like NaN): none -> NaN,
 *      otherwise the value at index n / 2 of the sorted values -- the upper median, the larger one for n = 2, what
 *      std::nth_element(begin, begin + n / 2, end) leaves there.  The result is one of the inputs bit for bit (where a window
 *      holds -0.0 and +0.0 around the median rank the sign of the zero is unspecified upstream; here -0.0 sorts below +0.0);
 *   4. fill mask               V = the cells finite in the input; C = V after k = num_erode_dilation_iterations erosions and
 *      then k dilations with a 3 x 3 square, where cells outside the map do not vote (an erosion keeps a cell whose in-map
 *      neighbours are all set, a dilation sets a cell with any in-map neighbour set); shouldFill(c) = some cell of C lies in
 *      c's window of radius r_fill.  With k = 0: "the window holds a finite value";
 *   5. per cell, reading only the input layer as it was before the call:
 *        input not finite and shouldFill                        -> median(r_fill)
 *        input finite, filter_existing_values and shouldFill    -> median(r_existing)   (radius 0: the identity)
 *        otherwise                                              -> the input value, bits unchanged (a NaN outside the mask stays);
 *   6. not built: the reuse of a fill_mask layer kept from an earlier update, and the debug layers.  Every call computes its mask.
 * Defaults as remembered from upstream: fill_hole_radius 0.05, filter_existing_values false, existing_value_radius 0.0,
 * num_erode_dilation_iterations 4.  Validation as configure(): radii finite and >= 0, iterations >= 0 (TE_ERR_BAD_PARAM + message). */
typedef struct te_median_fill_params {
  uint32_t size; /* sizeof(te_median_fill_params) */
  uint32_t abi_version;
  double fill_hole_radius;
  int32_t filter_existing_values;
  int32_t _pad0;
  double existing_value_radius;
  int32_t num_erode_dilation_iterations;
  int32_t _pad1;
} te_median_fill_params;
int te_median_fill_params_default(te_median_fill_params* p);
int te_median_fill_params_validate(const te_median_fill_params* p);
/* out_layer = MedianFillFilter(in_layer) for maps [map0, map0 + nmaps) of the batch; the other maps are untouched.  Any two float
 * layers of the context; the same layer in and out (the elevation filled in place) behaves as if the input had been copied
 * first -- the copy is taken from device memory on first use, TE_ERR_UNSUPPORTED if it does not fit.  Exact: the result is
 * identical run after run and between the two kernels (TE_OPT_MEDIAN_ROUTE).  Asynchronous on the context's stream unless
 * out_layer is the elevation.
 *   TE_ERR_NOT_READY: no geometry; an input layer that does not exist yet (an elevation never uploaded, the layers
 *     te_run_expression refuses to read).  TE_ERR_INVALID_ARG: NULL, a layer id out of range or without memory
 *     (traversability_x before te_run_polygon_footprint), a map range outside the batch.  TE_ERR_BAD_PARAM: the parameters.
 *     TE_ERR_UNSUPPORTED: the general kernel on a map of 2^32 cells or more.
 *   Afterwards the context holds what an upload of the same values into out_layer leaves.  TE_LAYER_ELEVATION: the pass of
 *     te_upload_elevation has run over the NEW contents -- invalid cells, their runs and the face flags are recounted, so a
 *     completely filled map takes the hole-free normals kernel and one that keeps holes takes their march -- the layer counts
 *     as uploaded, chain and footprint results as stale.  Any other layer: as te_upload_layer (traversability: no known bound;
 *     robot_slope: present; a score layer: the footprint mask is stale).
 *   A prefetch in flight that writes either layer is joined first. */
int te_run_median_fill(te_ctx* ctx, const te_median_fill_params* p, int in_layer, int out_layer, int map0, int nmaps);
/* The fill after in_layer changed inside the rectangle (row0, col0) + (h, w) of map `map` only (te_upload_layer_tile).
 *   Precondition: out_layer holds te_run_median_fill(p, in_layer, out_layer) of the EARLIER contents of in_layer -- from the
 *     whole-map call or from region calls since.  Postcondition: out_layer of that map equals, bit for bit, what the whole-map
 *     call would write now.  Only the cells of out_rect = {row0, col0, h, w} of the rectangle written are touched: the input
 *     rectangle grown by the reach and clamped to the map; other maps are untouched.  Reach, a Chebyshev distance:
 *     max(r_fill + 2 k, r_existing if filter_existing_values else 0), k = num_erode_dilation_iterations (k erosions and k
 *     dilations carry a change of V 2 k cells; cells outside the MAP do not vote, the region border is no map border).
 *     csrc/te_region_plan.h has every stage's rectangle.  Work and traffic are those of the region: nothing is sized by the map.
 *   te_download_fill_mask afterwards returns the whole-map mask of the updated input (the call refreshes out_rect of the stored
 *     mask) -- TE_ERR_NOT_READY if no te_run_median_fill of that map preceded: there is no mask to refresh.
 *   in_layer == out_layer: TE_ERR_INVALID_ARG -- in place the earlier input of the neighbouring cells is gone.  A rectangle
 *     outside the map, a bad map: TE_ERR_INVALID_ARG as te_run_chain_region.  Every other error as te_run_median_fill.
 *   Afterwards: out_layer == TE_LAYER_ELEVATION leaves exactly what te_upload_tile of out_rect leaves -- the done-flags stay,
 *     face flags and hole counts are unknown until the next whole upload -- and the next call is te_run_chain_region on out_rect.
 *     Any other out_layer: as te_upload_layer.  Asynchronous on the context's stream; a prefetch that writes either layer is
 *     joined first.  TE_OPT_MEDIAN_ROUTE steers it as it steers the whole-map call. */
int te_run_median_fill_region(te_ctx* ctx, const te_median_fill_params* p, int in_layer, int out_layer, int map, int row0, int col0, int h, int w,
                              int out_rect[4]);
/* shouldFill (4.) of the last te_run_median_fill that covered `map`: rows * cols bytes (exactly `bytes`) of 0 / 1, column-major
 * like the layers.  TE_ERR_NOT_READY before any such call and after every te_set_geometry. */
int te_download_fill_mask(te_ctx* ctx, int map, unsigned char* out, size_t bytes);
/* Measurement aid (tools/median_fill_bench.py): `iters` launches, one HIP event pair each, ms[k] = device time of the k-th after
 * `warmup` untimed ones.  p != NULL: te_run_median_fill(p, in_layer, out_layer) over the whole batch, without the recount that
 * follows a fill of the elevation (the input must survive the repeats: in_layer != out_layer is required).  p == NULL: a device
 * copy of in_layer into out_layer, the fill's floor. */
int te_time_median_fill_samples(te_ctx* ctx, const te_median_fill_params* p, int in_layer, int out_layer, int warmup, int iters, float* ms);

/* ---- gridMapFilters/MeanInRadiusFilter and MinInRadiusFilter on the device: smoothing and the lower surface ----
 * Like the median fill this contract is RESTATED from memory of grid_map_filters; nothing the reference holds pins it.  The
 * yardstick of the tests is the same contract in numpy (tests/ref_py/radius_filter_ref.py).
 *   1. disc            for every cell c of the map (valid or not): center = getPosition(c), the window is
 *      CircleIterator(map, center, radius) -- the disc of csrc/te_disc_table.h: cells outside the map are no cells, cells on
 *      the circle are decided per centre with the reference's double arithmetic.  The same disc as StepFilter's first window;
 *   2. iteration order row index ascending outer, column index ascending inner;
 *   3. values used     a value takes part iff std::isfinite(value): +-inf is skipped like NaN;
 *   4. Mean            double sum = 0.0; int n = 0; over the window in that order: sum += (double)value; ++n.  The output is
 *      (float)(sum / n) for n > 0, else NaN (the freshly added layer).  Defined bit for bit, including where partial sums round
 *      (a disc of -0.0 cells gives +0.0);
 *   5. Min             the smallest finite value of the window, NaN if there is none: one of the inputs, bit for bit.  Where a
 *      window holds -0.0 and +0.0 as its minimum upstream's sign depends on the order; here -0.0 sorts below +0.0;
 *   6. parameters      radius, input_layer, output_layer.  The radius must be finite and >= 0 (TE_ERR_BAD_PARAM + message);
 *      radius 0 is the centre cell alone;
 *   7. the same layer in and out behaves as if the input had been copied first (what upstream does with equal names is not
 *      restated). */
#define TE_RADIUS_MEAN 1
#define TE_RADIUS_MIN 2
/* out_layer = the Mean / Min in `radius` of in_layer for maps [map0, map0 + nmaps) of the batch; the other maps are untouched.
 * Any two float layers of the context, any radius: the call owns its disc table and does not depend on
 * TE_OPT_FILTER_ANY_RADIUS.  Exact: identical run after run and between the kernels (TE_OPT_RADIUS_ROUTE).  The Mean's sliding
 * kernel adds column prefix sums -- another order than 2. -- and a workgroup takes it only where the order provably cannot
 * matter (csrc/te_radius_plan.h: order_free over the exponents of the cells it reads); otherwise the workgroup walks its windows
 * in order.  Asynchronous on the context's stream unless out_layer is the elevation.
 *   TE_ERR_NOT_READY, TE_ERR_INVALID_ARG (also: an op that is neither), TE_ERR_BAD_PARAM (the radius), the context afterwards and
 *   the joining of a prefetch: as te_run_median_fill.  TE_ERR_UNSUPPORTED: the window table or the copy of the input layer does
 *   not fit in device memory. */
int te_run_radius_filter(te_ctx* ctx, int op, double radius, int in_layer, int out_layer, int map0, int nmaps);
/* The Mean / Min after in_layer changed inside the rectangle of map `map` only: the contract of te_run_median_fill_region with
 * te_run_radius_filter in the place of the fill.  Reach: that of the disc table the whole-map call builds for `radius`
 * (csrc/te_disc_table.h; 0, 1, 2, 3, 9 cells at 0, 1.5, 2.0, 3 and 9 cells of radius); the table is kept from call to call.  The
 * sliding Mean decides order_free per workgroup of ITS tiling, which starts at out_rect's corner; a workgroup that passes adds
 * exactly, so the bits are the whole-map call's.  te_radius_filter_stats counts the region call's workgroups.
 * TE_OPT_RADIUS_ROUTE steers it as it steers the whole-map call. */
int te_run_radius_filter_region(te_ctx* ctx, int op, double radius, int in_layer, int out_layer, int map, int row0, int col0, int h, int w,
                                int out_rect[4]);
/* Which kernel the last te_run_radius_filter ran: counts[0] = workgroups the sliding kernel settled, counts[1] = workgroups the
 * in-order gather settled (the gather kernel's own, and those of the sliding Mean that failed the predicate).  Waits for the
 * call.  TE_ERR_NOT_READY before any call. */
int te_radius_filter_stats(te_ctx* ctx, uint64_t counts[2]);
/* Measurement aid (tools/radius_filter_bench.py), like te_time_median_fill_samples: `iters` launches over the whole batch, one
 * HIP event pair each, after `warmup` untimed ones; in_layer != out_layer is required.  op = 0: a device copy of the layer. */
int te_time_radius_filter_samples(te_ctx* ctx, int op, double radius, int in_layer, int out_layer, int warmup, int iters, float* ms);

/* ---- The clearance layer: the exact Euclidean distance of every cell to the nearest seed of its map ----
 * Unlike the filters above this one is DEFINED here, not restated: it is arithmetic, and a brute-force loop over all pairs
 * (tests/ref_py/distance_ref.py) pins every bit.  Unsigned, one threshold, 2-D.
 *   1. seeds           a cell v of in_layer is a seed iff v < (float)threshold (TE_DISTANCE_BELOW) or v > (float)threshold
 *      (TE_DISTANCE_ABOVE): ThresholdFilter's comparisons, so v == threshold is a seed in neither mode.  A NaN cell is a seed
 *      iff TE_DISTANCE_NAN_IS_SEED is or-ed in; without it a NaN cell is an ordinary cell and gets its distance;
 *   2. d2              for every cell the smallest di * di + dj * dj (an integer, in cells) over the seeds of the same map;
 *   3. cap             res = the map's resolution (double); cap2 = the largest integer k with
 *      (double)k * (res * res) <= max_distance * max_distance; the reach R = floor(sqrt(cap2)) cells;
 *   4. output          a seed gets 0.0f; a cell with d2 <= cap2 gets (float)(sqrt((double)d2) * res); every other cell -- a map
 *      without a seed included -- gets (float)max_distance.  The output never holds a NaN.  With cell-centred discs, "the disc
 *      of radius r <= max_distance around this cell holds a seed" is output <= r;
 *   5. parameters      max_distance must be finite and positive with R <= 32767, the threshold finite (TE_ERR_BAD_PARAM + message).
 * Two separable passes, both exact in integers; nothing is decided in floating point before the final sqrt. */
#define TE_DISTANCE_BELOW 1      /* seed iff v < (float)threshold   (ThresholdFilter's comparisons) */
#define TE_DISTANCE_ABOVE 2      /* seed iff v > (float)threshold */
#define TE_DISTANCE_NAN_IS_SEED 4 /* or-ed in: a NaN cell is a seed too; without it a NaN cell is never one */
/* out_layer = the distance layer of in_layer for maps [map0, map0 + nmaps) of the batch; the other maps are untouched.  Any two
 * float layers of the context, user layers included; in_layer == out_layer needs no copy.  Identical run after run and between
 * the routes (TE_OPT_DISTANCE_ROUTE).  Asynchronous on the context's stream unless out_layer is the elevation.
 *   TE_ERR_INVALID_ARG (also: a mode that is neither comparison), TE_ERR_NOT_READY, the context afterwards and the joining of a
 *   prefetch: as te_run_radius_filter.  TE_ERR_BAD_PARAM: 5.  TE_ERR_UNSUPPORTED: the scratch of the first pass (2 bytes per
 *   cell of the call) does not fit in device memory. */
int te_run_distance(te_ctx* ctx, int mode, double threshold, double max_distance, int in_layer, int out_layer, int map0, int nmaps);
/* The distance layer after in_layer changed inside the rectangle of map `map` only: the contract of te_run_radius_filter_region
 * with the reach R of 3.  out_rect = the rectangle grown by R and clamped to the map; what the call writes there is bit for bit
 * what the whole-map call would write, and no other cell is touched.  It reads no cell of in_layer farther than 2 R from the
 * rectangle, and no launch and no scratch is sized by the map.  in_layer == out_layer: TE_ERR_INVALID_ARG. */
int te_run_distance_region(te_ctx* ctx, int mode, double threshold, double max_distance, int in_layer, int out_layer, int map, int row0, int col0, int h,
                           int w, int out_rect[4]);
/* Which route the second pass of the last te_run_distance or te_run_distance_region took: counts[0] = its workgroups on the
 * tiled route, counts[1] = on the route of any reach.  TE_ERR_NOT_READY before any call. */
int te_distance_stats(te_ctx* ctx, uint64_t counts[2]);
/* Measurement aid (tools/distance_bench.py), like te_time_radius_filter_samples: `iters` launches over the whole batch, one HIP
 * event pair each, after `warmup` untimed ones; in_layer != out_layer is required.  mode = 0: a device copy of the layer.  One
 * of the two bits below or-ed into a mode times that pass alone (the second on the column distances of one untimed first
 * pass); out_layer then holds no distance layer if it is the first. */
#define TE_DISTANCE_TIME_PASS1 0x100
#define TE_DISTANCE_TIME_PASS2 0x200
int te_time_distance_samples(te_ctx* ctx, int mode, double threshold, double max_distance, int in_layer, int out_layer, int warmup, int iters, float* ms);

/* ---- Connected regions: the components of the free cells of a map, their sizes, and what a set of start cells reaches ----
 * Like the clearance layer this is DEFINED here, not restated: a brute-force flood fill (tests/ref_py/components_ref.py) is the
 * definition, the result is unique, and the device is held to it bit for bit.
 *   1. blocked / free  a cell v of in_layer is blocked iff it is a seed of te_run_distance under the same mode and threshold
 *      (TE_DISTANCE_BELOW / TE_DISTANCE_ABOVE, TE_DISTANCE_NAN_IS_SEED or-ed in, compared on the float; v == threshold is blocked
 *      in neither mode).  Every other cell is free; without the NaN bit a NaN cell is free;
 *   2. neighbours      connectivity 4: (i +- 1, j) and (i, j +- 1); 8: those and the four diagonals, and a diagonal step
 *      connects two free cells whatever the two cells beside it are.  No wrap at the map border, no link between the maps of
 *      a batch.  Any other value: TE_ERR_INVALID_ARG;
 *   3. components      the classes of the free cells of one map under the transitive closure of 2;
 *   4. sizes           te_run_components: a free cell gets (float)n, n the number of cells of its component as a 32-bit unsigned
 *      integer converted to float, round to nearest (exact up to 2^24); a blocked cell gets 0.0f;
 *   5. reachable       te_run_reachable: a free cell whose component holds at least one start cell gets 1.0f, every other cell
 *      -- blocked ones included -- 0.0f, so traversability .* reachable is a planner's map.  A start on a blocked cell reaches
 *      nothing.
 * Limits: no region form (one changed cell can merge or split components anywhere), no chain-file type, no C++ plugin; the
 * labels themselves are not exposed; v == threshold is free, so for "clearance <= r is blocked" pass the next float above r
 * with TE_DISTANCE_BELOW. */
#define TE_COMPONENTS_CONNECTIVITY_4 4
#define TE_COMPONENTS_CONNECTIVITY_8 8
#define TE_REACHABLE_MAX_STARTS 256
/* out_layer = the size layer (4) of in_layer for maps [map0, map0 + nmaps) of the batch; the other maps are untouched.  Any two
 * float layers of the context, user layers included; in_layer == out_layer needs no copy.  Identical run after run.
 * Asynchronous on the context's stream unless out_layer is the elevation.
 *   TE_ERR_INVALID_ARG (also: a mode that is neither comparison, a connectivity that is neither 4 nor 8), TE_ERR_NOT_READY, the
 *   context afterwards and the joining of a prefetch: as te_run_distance.  TE_ERR_BAD_PARAM: a threshold that is not finite.
 *   TE_ERR_UNSUPPORTED: a map of 2^31 cells or more, or the scratch (8 bytes per cell of the call) does not fit in device memory. */
int te_run_components(te_ctx* ctx, int mode, double threshold, int connectivity, int in_layer, int out_layer, int map0, int nmaps);
/* out_layer = the reachable layer (5) of map `map` of in_layer from the n_starts cells start_cells[2 k] = row, [2 k + 1] = column;
 * layers, errors and the stream as te_run_components.  n_starts must be in [1, TE_REACHABLE_MAX_STARTS] and start_cells not NULL;
 * a start outside the map: TE_ERR_INVALID_ARG, and nothing is written.  The starts are copied before the call returns. */
int te_run_reachable(te_ctx* ctx, int mode, double threshold, int connectivity, int in_layer, int out_layer, int map, int n_starts, const int* start_cells /* row, col pairs */);
/* The last te_run_components or te_run_reachable, over all its maps: counts[0] = components, counts[1] = free cells, counts[2] =
 * cells of the largest component, counts[3] = cells written 1.0f (0 after te_run_components).  Unlike te_distance_stats the
 * values come from the device: the call waits for the context's stream and reads 32 bytes.  TE_ERR_NOT_READY before any call. */
int te_components_stats(te_ctx* ctx, uint64_t counts[4]);

/* ---- gridMapFilters/SlidingWindowMathExpressionFilter on the device: an expression over a window around every cell ----
 * Like the median fill and the radius filters this contract is RESTATED from memory of grid_map_filters and EigenLab; nothing
 * the reference holds pins it.  The yardstick of the tests is the same contract in numpy (tests/ref_py/window_expression_ref.py).
 *   1. parameters      input_layer, output_layer, expression; exactly one of window_size (int) and window_length (double,
 *      metres); compute_empty_cells (default true); edge_handling in inside | crop | empty | mean (default inside).
 *   2. window size     window_size is taken as given.  With window_length: w = (int)std::round(window_length / resolution) (a
 *      double division, halves away from zero), then ++w if w is even.  w must be odd and at least 1 (upstream throws; here
 *      TE_ERR_BAD_PARAM + message, also for a length that is negative or not finite).  Margin m = (w - 1) / 2.
 *   3. the window of cell (i, j): rows [i - m, i + m], columns [j - m, j + m]; B is that rectangle clipped to the map.
 *        inside   a cell whose rectangle is not wholly inside the map is not visited;
 *        crop     the window W is B, smaller near the border;
 *        empty    W is w x w, NaN outside the map;
 *        mean     W is w x w; outside the map it holds the float32 meanOfFinites(B) by rule 5 (NaN if B has no finite value);
 *        compute_empty_cells == false: a cell whose own input value is not finite is not visited.
 *      A cell that is not visited gets NaN.  The whole output layer of the covered maps is written (upstream add()s it first).
 *   4. the expression  the language of te_run_expression with three differences: (a) the only variable is the input layer,
 *      written by its name, and it denotes W (any other layer name: TE_ERR_BAD_PARAM); (b) the result must be a scalar -- a
 *      main expression that leaves a map, like abs(elevation), is refused when it is compiled (TE_ERR_BAD_PARAM; upstream logs
 *      an error per cell and leaves NaN); (c) reductions nest ONE level: a reduction's argument may hold reductions whose own
 *      arguments hold none (deeper: TE_ERR_BAD_PARAM).  At most 4 reductions and 64 instructions in all.  Scalar .* ./ ^ as
 *      in te_run_expression; * between two maps stays TE_ERR_UNSUPPORTED.  A scalar argument of a reduction counts once per
 *      cell of W, as it counts once per cell of the map there.
 *   5. reductions over W, defined bit for bit: every column of W in ascending column order yields a partial -- a double sum
 *      starting at 0.0 over the rows in ascending order (and minimum, maximum and count of the finite values); the column
 *      partials are folded in ascending column order into an empty partial (sum += sum); the result is taken from that with
 *      cells = rows(W) * cols(W).  sum and mean take every value (a NaN poisons them), the ...OfFinites kinds skip the
 *      non-finite ones.  Eigen's own redux order depends on its vectorisation and is not restated.
 *   6. the same layer in and out behaves as if the input had been copied first. */
#define TE_EDGE_INSIDE 0
#define TE_EDGE_CROP 1
#define TE_EDGE_EMPTY 2
#define TE_EDGE_MEAN 3
typedef struct te_window_expr_params {
  uint32_t size; /* sizeof(te_window_expr_params) */
  uint32_t abi_version;
  int32_t window_size;       /* odd, >= 1; 0 with use_window_length */
  int32_t use_window_length; /* 0: window_size, 1: window_length */
  double window_length;      /* metres; 0 without use_window_length */
  int32_t compute_empty_cells;
  int32_t edge_handling; /* TE_EDGE_* */
} te_window_expr_params;
/* Defaults: window_size 3 (upstream has none: one of the two must be given), compute_empty_cells 1, TE_EDGE_INSIDE. */
int te_window_expr_params_default(te_window_expr_params* p);
/* TE_ERR_INVALID_ARG: NULL, size / abi mismatch.  TE_ERR_BAD_PARAM + message: an even window_size or one below 1, both or
 * neither of window_size and window_length, a length that is negative or not finite, an edge_handling that is none of the four. */
int te_window_expr_params_validate(const te_window_expr_params* p);
/* Host only, no context: compiles `text` as a window expression over in_layer and describes it (`info` may be NULL).  Errors as
 * te_expr_check, the message with the column. */
int te_window_expr_check(const char* text, int in_layer, te_expr_info* info);
/* out_layer = the expression over the window of every cell of in_layer, for maps [map0, map0 + nmaps) of the batch; the other
 * maps are untouched.  Any two float layers of the context, any window.  Exact: identical run after run and between the
 * routes (TE_OPT_WINDOW_EXPR_ROUTE): the direct walk is rule 5 literally, O(w^2) per cell; the separable route keeps the column
 * partials of a tile in LDS and folds them per cell in rule 5's order, O(w) per cell.  The transcendental functions are the
 * device's, as in te_run_expression.  Asynchronous on the context's stream unless out_layer is the elevation.
 *   TE_ERR_NOT_READY, TE_ERR_INVALID_ARG, the context afterwards (the recount when the elevation is written included) and the
 *   joining of a prefetch: as te_run_radius_filter.  TE_ERR_BAD_PARAM: the parameters, the window, the expression.
 *   TE_ERR_UNSUPPORTED: valid EigenLab that is not built; the copy of the input layer does not fit in device memory. */
int te_run_window_expression(te_ctx* ctx, const te_window_expr_params* p, const char* text, int in_layer, int out_layer, int map0, int nmaps);
/* The window expression after in_layer changed inside the rectangle (row0, col0) + (h, w) of map `map` only
 * (te_upload_layer_tile): the contract of te_run_median_fill_region with the expression in the place of the fill.
 *   Precondition: out_layer holds te_run_window_expression(p, text, in_layer, out_layer) of the EARLIER contents of in_layer --
 *     from the whole-map call or from region calls since.  Postcondition: out_layer of that map equals, bit for bit, what the
 *     whole-map call would write now.  Only the cells of out_rect = {row0, col0, h, w} of the rectangle written are touched:
 *     the input rectangle grown by the reach and clamped to the map; other maps are untouched.
 *   Reach, a Chebyshev distance: m = (w - 1) / 2 cells under all four edge handlings.  A cell reads its window and nothing
 *     else.  Under TE_EDGE_MEAN the padding of a clipped window is meanOfFinites(B), and B -- the window clipped to the map --
 *     lies inside the window: the reach stays m.  Under TE_EDGE_INSIDE the unvisited frame inside out_rect gets its NaN again;
 *     with compute_empty_cells == 0 a cell whose own input is not finite gets NaN.  The region border is no map border: every
 *     read is checked against the map.  csrc/te_region_plan.h has the plan; the tiling starts at out_rect's corner.  Work and
 *     traffic are those of the region: no copy of the input layer, nothing is sized by the map.
 *   in_layer == out_layer: TE_ERR_INVALID_ARG -- in place the earlier input of the neighbouring cells is gone.  A rectangle
 *     outside the map, a bad map: TE_ERR_INVALID_ARG as te_run_chain_region.  Every other error as te_run_window_expression.
 *   Afterwards: out_layer == TE_LAYER_ELEVATION leaves exactly what te_upload_tile of out_rect leaves, and the next call is
 *     te_run_chain_region on out_rect.  Any other out_layer: as te_upload_layer_tile.  Asynchronous on the context's stream; a
 *     prefetch that writes either layer is joined first.  TE_OPT_WINDOW_EXPR_ROUTE steers it as it steers the whole-map call
 *     (both routes, the same bits), and te_window_expression_stats then counts the region call's workgroups. */
int te_run_window_expression_region(te_ctx* ctx, const te_window_expr_params* p, const char* text, int in_layer, int out_layer, int map, int row0,
                                    int col0, int h, int w, int out_rect[4]);
/* Which route the last te_run_window_expression took: counts[0] = workgroups the separable route settled, counts[1] =
 * workgroups that walked their windows directly.  Waits for the call.  TE_ERR_NOT_READY before any call. */
int te_window_expression_stats(te_ctx* ctx, uint64_t counts[2]);
/* Measurement aid (tools/window_expression_bench.py), like te_time_radius_filter_samples: `iters` launches over the whole
 * batch, one HIP event pair each, after `warmup` untimed ones; in_layer != out_layer is required.  p == NULL or text == NULL: a
 * device copy of the layer. */
int te_time_window_expression_samples(te_ctx* ctx, const te_window_expr_params* p, const char* text, int in_layer, int out_layer, int warmup, int iters, float* ms);

const char* te_last_error(void);
const char* te_version(void);

#ifdef __cplusplus
}
#endif
#endif /* TRAVGPU_H */
