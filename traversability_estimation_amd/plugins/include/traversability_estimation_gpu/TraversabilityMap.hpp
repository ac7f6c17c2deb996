/*
 * TraversabilityMap.hpp -- device-backed counterpart of traversability_estimation::TraversabilityMap
 * (traversability_estimation/include/traversability_estimation/TraversabilityMap.hpp) for the part of it that is the
 * hot path: filter chain, footprint layers and footprint-path checks.  Same method names, argument meaning and return
 * conventions; the map stays on the device between calls (its own te_ctx), layers come back only through
 * getTraversabilityMap().  What a maintainer swaps in for the members of the ROS node that do the arithmetic
 * (TraversabilityMap.cpp:156-237, 239-318, 320-645); node handle, publishers, services and tf stay where they are.
 */
#ifndef TRAVERSABILITY_ESTIMATION_GPU_TRAVERSABILITYMAP_HPP
#define TRAVERSABILITY_ESTIMATION_GPU_TRAVERSABILITYMAP_HPP

#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include <grid_map_core/GridMap.hpp>
#include <nav_msgs/OccupancyGrid.h>
#include <sensor_msgs/Image.h>
#include <sensor_msgs/PointCloud2.h>
#include <traversability_msgs/FootprintPath.h>
#include <traversability_msgs/TraversabilityResult.h>

#include "travgpu.h"

namespace traversability_estimation_gpu {

class TraversabilityMap {
 public:
  explicit TraversabilityMap(int device = 0);
  ~TraversabilityMap();
  TraversabilityMap(const TraversabilityMap&) = delete;
  TraversabilityMap& operator=(const TraversabilityMap&) = delete;

  /*! Filter and footprint parameters (the YAML of the reference: robot_filter_parameter.yaml,
   *  robot_footprint_parameter.yaml, robot.yaml); false + error() if the reference's configure() would refuse them. */
  bool setParameters(const te_params& params);
  const te_params& getParameters() const { return params_; }
  /*! footprint/footprint_polygon (TraversabilityMap.cpp:91-103). */
  void setFootprintPolygon(const std::vector<geometry_msgs::Point32>& points) { footprintPoints_ = points; }

  /*! footprint/check_robot_inclination (:114): checkFootprintPath then runs checkInclination (:748-762) on the layer
   *  "robot_slope" of the elevation map handed to setElevationMap (the path checks fail if it had none). */
  bool setCheckRobotInclination(bool enabled);
  /*! setElevationMap (:135-154): needs the layer "elevation"; any start index.  A layer "robot_slope" goes along. */
  bool setElevationMap(const grid_map::GridMap& elevationMap);
  /*! imageCallback's body (TraversabilityEstimation.cpp:154-168) on the device: initializeFromImage -- the map takes the
   *  image's size (rows = height, cols = width), `resolution` and `position` -- then addLayerFromImage(image, "elevation",
   *  map, minHeight, maxHeight).  The image's own bytes cross PCIe (te_upload_image); computeTraversability() then works
   *  from it as it does after setElevationMap.  False + error() for an encoding grid_map_ros refuses or a data size that is
   *  not step * height.  An image carries no layer "robot_slope". */
  bool setElevationFromImage(const sensor_msgs::Image& image, double resolution, const grid_map::Position& position,
                             double minHeight, double maxHeight);
  /*! GridMap::move on the device (te_move_map): the resident map follows the robot to `position`, rounded to whole cells,
   *  without a new setElevationMap.  `info` receives the plan: the shift, the position held afterwards and up to four
   *  rectangles (row0, col0, h, w).  exposedCells[k], for a rectangle k with info.rect_exposed[k] == 1, points to its h x w new
   *  elevation cells, column-major like a GridMap block (nullptr, or no array at all: the cells stay NaN).  The loop of
   *  INTEGRATION.md "Incremental updates of a resident map" then runs: each strip is uploaded and, if the traversability map
   *  was computed, every rectangle -- the trailing border lines included -- is re-filtered (te_run_chain_region), or the
   *  whole chain runs when info.results_kept == 0 (a tie radius, raster normals); a circular footprint layer that existed is
   *  rebuilt by one whole-map footprint pass (include/travgpu.h, caveat 3); the polygon layers are dropped.  A zero shift
   *  changes nothing.  false + error(), and nothing moved, without an elevation map or with setFillHoles / setSmoothElevation
   *  in force (the strips would enter the elevation layer raw: use the region forms of the C API). */
  bool moveMap(const grid_map::Position& position, te_move_info& info, const float* const* exposedCells = nullptr);
  /*! computeTraversability (:202-237): the filter chain; false if no elevation map has been set. */
  bool computeTraversability();
  /*! Hole filling in front of the chain (gridMapFilters/MedianFillFilter on the device, te_run_median_fill): with parameters
   *  set, computeTraversability() first fills the resident elevation layer in place -- once per elevation map -- and the chain
   *  then sees a layer without the holes that had observed neighbours.  NULL switches it off again (the default).  false (and
   *  nothing changed) for parameters te_median_fill_params_validate refuses. */
  bool setFillHoles(const te_median_fill_params* params);
  /*! Smoothing in front of the chain (gridMapFilters/MeanInRadiusFilter on the device, te_run_radius_filter): with a radius
   *  above 0, computeTraversability() replaces the resident elevation layer by its mean within that radius -- once per
   *  elevation map, after the hole filling of setFillHoles -- and the chain sees the smoothed layer.  0 switches it off again
   *  (the default).  false (and nothing changed) for a radius that is negative or not finite. */
  bool setSmoothElevation(double radius);
  /*! NormalVectorsFilter's `algorithm` of robot_filter_parameter.yaml: false the area method (the default), true the raster
   *  method (te_set_option TE_OPT_NORMALS_ALGORITHM: the normal from the finite differences of a cell's four neighbours;
   *  normals_radius then plays no part).  The next computeTraversability() runs it; results computed so far are dropped. */
  bool setNormalsAlgorithm(bool raster);
  /*! traversabilityFootprint(radius, offset) (:307-318): layer traversability_footprint. */
  bool traversabilityFootprint(const double& radius, const double& offset);
  /*! traversabilityFootprint(footprintYaw) (:239-305): layers traversability_x / traversability_rot. */
  bool traversabilityFootprint(double footprintYaw);
  /*! checkFootprintPath (:320-342): circular footprint when path.footprint has no points, else polygonal.  Returns
   *  false only for a path without poses; an uninitialised map gives is_safe = false and true, like the reference. */
  bool checkFootprintPath(const traversability_msgs::FootprintPath& path, traversability_msgs::TraversabilityResult& result);
  /*! The CheckFootprintPath service body (TraversabilityEstimation.cpp:276-291) for all paths of a request at once:
   *  one device launch per footprint kind.  Returns false if any path has no poses (its result stays unsafe). */
  bool checkFootprintPaths(const std::vector<traversability_msgs::FootprintPath>& paths,
                           std::vector<traversability_msgs::TraversabilityResult>& results);
  /*! How circular paths are checked.  Off (the default): per distinct radius of the request a whole-map footprint pass at
   *  that radius, then the path kernel on the layer -- traversability_footprint and the footprint radius of the parameters
   *  then belong to the last path check.  On: every circular path of the request goes through ONE call with its own
   *  path.radius, evaluated on demand at the centres it visits (te_check_footprint_paths_radius), as the reference does
   *  (:345-462 with isTraversable's on-demand branch); the layer a traversabilityFootprint(radius, offset) call computed and
   *  the parameters stay as they are. */
  void setPathCheckOnDemand(bool enabled) {
    std::lock_guard<std::mutex> lock(mutex_);
    pathCheckOnDemand_ = enabled;
  }
  /*! The elevation map's geometry with the layers computed so far (getTraversabilityMap :196-199). */
  grid_map::GridMap getTraversabilityMap();
  /*! GridMapRosConverter::toOccupancyGrid(map, layer, dataMin, dataMax, grid) on the device, for the layers
   *  getTraversabilityMap() would return (config/visualization/traversability.yaml: the four score layers with dataMin 1,
   *  dataMax 0): one byte per cell crosses PCIe (te_download_occupancy).  The caller stamps grid.header BEFORE the call:
   *  info.map_load_time is set to that stamp, as toOccupancyGrid does.  False + error() for a layer that is not there. */
  bool getOccupancyGrid(const std::string& layer, float dataMin, float dataMax, nav_msgs::OccupancyGrid& grid);
  /*! GridMapRosConverter::toPointCloud(map, layers, pointLayer, cloud) on the device: only the cells whose point layer is
   *  finite cross PCIe (te_download_cloud).  pointLayer must be one of `layers`. */
  bool getPointCloud(const std::vector<std::string>& layers, const std::string& pointLayer, sensor_msgs::PointCloud2& cloud);
  /*! The get_traversability service body (TraversabilityEstimation.cpp:297-316) on the device: `message` receives the ROS1
   *  serialisation of the grid_map_msgs/GridMap that toMessage(getTraversabilityMap().getSubmap(position, length), layers)
   *  gives -- the submap's own geometry, start index (0, 0) -- and only the rectangle of the named layers crosses PCIe
   *  (te_download_submap_msg).  An empty `layers` names every layer getTraversabilityMap() would return, as the service does.
   *  `header` (may be null) gives seq, stamp, frame_id, pose z and orientation.  Returns getSubmap's isSuccess: false with an
   *  empty message and an empty error() for a request getSubmap refuses, false + error() for a layer that is not there. */
  bool getTraversabilityMap(const grid_map::Position& position, const grid_map::Length& length, const std::vector<std::string>& layers,
                            std::vector<uint8_t>& message, const te_msg_info* header = nullptr);
  bool traversabilityMapInitialized() const { return traversabilityMapInitialized_; }
  const std::string& error() const { return error_; }

 private:
  bool check(int rc);
  bool ensureCircularFootprint(double radius);
  int deviceLayer(const std::string& name) const;  // te_layer of a layer getTraversabilityMap() would return, else -1
  mutable std::mutex mutex_;
  te_ctx* ctx_;
  te_params params_;
  te_median_fill_params fillParams_;
  bool fillHoles_, elevationFilled_;  // setFillHoles; the resident elevation has been filled with fillParams_
  double smoothRadius_;               // setSmoothElevation (0: off)
  bool elevationSmoothed_;            // the resident elevation has been smoothed with smoothRadius_
  std::vector<geometry_msgs::Point32> footprintPoints_;
  grid_map::GridMap geometry_;  // geometry and start index of the last elevation map (no layers)
  bool elevationMapInitialized_, traversabilityMapInitialized_, footprintLayer_, polygonLayers_;
  bool checkRobotInclination_, robotSlopeLayer_;
  bool pathCheckOnDemand_ = false;
  double footprintRadius_, footprintOffset_;
  double circularFootprintOffset_;  // :348 "TODO: get this with FootprintPath msg" = 0.15
  std::string error_;
};

}  // namespace traversability_estimation_gpu
#endif
