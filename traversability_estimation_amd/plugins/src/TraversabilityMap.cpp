#include "traversability_estimation_gpu/TraversabilityMap.hpp"

#include <cmath>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include <ros/ros.h>

namespace traversability_estimation_gpu {

TraversabilityMap::TraversabilityMap(int device)
    : ctx_(nullptr),
      elevationMapInitialized_(false),
      traversabilityMapInitialized_(false),
      footprintLayer_(false),
      polygonLayers_(false),
      checkRobotInclination_(false),
      robotSlopeLayer_(false),
      footprintRadius_(-1.0),
      footprintOffset_(-1.0),
      circularFootprintOffset_(0.15) {
  te_params_default(&params_);
  te_median_fill_params_default(&fillParams_);
  fillHoles_ = elevationFilled_ = false;
  smoothRadius_ = 0.0;
  elevationSmoothed_ = false;
  // (the reference's filters take any radius: TE_OPT_FILTER_ANY_RADIUS = 1)
  if (check(te_create(device, &ctx_))) {
    if (check(te_set_option(ctx_, TE_OPT_FILTER_ANY_RADIUS, 1))) {
      check(te_set_params(ctx_, &params_));
    } else {
      te_destroy(ctx_);  // (no context without the option)
      ctx_ = nullptr;
    }
  }
}

TraversabilityMap::~TraversabilityMap() {
  if (ctx_) te_destroy(ctx_);
}

bool TraversabilityMap::check(int rc) {
  if (rc == TE_OK) return true;
  error_ = te_last_error();
  ROS_ERROR("TraversabilityMap (MI355X): %s", error_.c_str());
  return false;
}

bool TraversabilityMap::setParameters(const te_params& params) {
  std::lock_guard<std::mutex> lock(mutex_);
  if (!ctx_ || !check(te_set_params(ctx_, &params))) return false;
  params_ = params;
  traversabilityMapInitialized_ = false;  // conservative: computeTraversability() has to run again
  footprintLayer_ = polygonLayers_ = false;
  return true;
}

bool TraversabilityMap::setCheckRobotInclination(bool enabled) {
  std::lock_guard<std::mutex> lock(mutex_);
  if (!ctx_ || !check(te_set_check_robot_inclination(ctx_, enabled ? 1 : 0))) return false;
  checkRobotInclination_ = enabled;
  return true;
}

bool TraversabilityMap::setElevationMap(const grid_map::GridMap& elevationMap) {
  std::lock_guard<std::mutex> lock(mutex_);
  if (!ctx_) return false;
  if (!elevationMap.exists("elevation")) {  // :145-150
    ROS_WARN("Traversability Map: Can't set elevation map because there is no layer %s.", "elevation");
    return false;
  }
  const int rows = elevationMap.getSize()(0), cols = elevationMap.getSize()(1);
  if (!check(te_set_geometry(ctx_, rows, cols, 1, elevationMap.getResolution(), elevationMap.getPosition().x(),
                             elevationMap.getPosition().y())))
    return false;
  const auto start = elevationMap.getStartIndex();
  if (!check(te_upload_layer_circular(ctx_, TE_LAYER_ELEVATION, elevationMap.get("elevation").data(), 0, start(0), start(1))))
    return false;
  // robot_slope (robotSlopeType_ :47) is nowhere computed by the reference: checkInclination reads it off whatever map
  // the node was handed, so it travels with the elevation map when it is there
  robotSlopeLayer_ = elevationMap.exists("robot_slope");
  if (robotSlopeLayer_) {
    if (!check(te_upload_layer_circular(ctx_, TE_LAYER_ROBOT_SLOPE, elevationMap.get("robot_slope").data(), 0, start(0), start(1))))
      return false;
  } else {
    // a map without the layer: the device must not keep checking inclinations against the previous map's layer (the
    // reference's atPosition("robot_slope") throws for a map that lacks it)
    (void)te_set_layer_present(ctx_, TE_LAYER_ROBOT_SLOPE, 0);
  }
  geometry_ = grid_map::GridMap();
  geometry_.setGeometry(elevationMap.getLength(), elevationMap.getResolution(), elevationMap.getPosition());
  geometry_.setStartIndex(start);
  elevationMapInitialized_ = true;
  elevationFilled_ = elevationSmoothed_ = false;
  traversabilityMapInitialized_ = false;
  footprintLayer_ = polygonLayers_ = false;
  return true;
}

bool TraversabilityMap::setElevationFromImage(const sensor_msgs::Image& image, double resolution, const grid_map::Position& position,
                                              double minHeight, double maxHeight) {
  std::lock_guard<std::mutex> lock(mutex_);
  if (!ctx_) return false;
  // the encodings grid_map_ros's addLayerFromImage takes (its switch on the cv type): channels, bytes per channel
  static const std::map<std::string, std::pair<int, int>> layouts = {
      {"mono8", {1, 1}},  {"8UC1", {1, 1}},  {"mono16", {1, 2}}, {"16UC1", {1, 2}},  {"rgb8", {3, 1}},   {"bgr8", {3, 1}},
      {"8UC3", {3, 1}},   {"rgba8", {4, 1}}, {"bgra8", {4, 1}},  {"8UC4", {4, 1}},   {"rgb16", {3, 2}},  {"bgr16", {3, 2}},
      {"16UC3", {3, 2}},  {"rgba16", {4, 2}}, {"bgra16", {4, 2}}, {"16UC4", {4, 2}}};
  const auto layout = layouts.find(image.encoding);
  if (layout == layouts.end()) {
    error_ = "setElevationFromImage: encoding '" + image.encoding + "'";
    ROS_ERROR("Expected MONO8, MONO16, RGB(A)8, RGB(A)16, BGR(A)8, or BGR(A)16 image encoding.");
    return false;
  }
  if (image.height == 0 || image.width == 0 || image.height > 0x7fffffffu || image.width > 0x7fffffffu || image.step > 0x7fffffffu ||
      image.data.size() != (size_t)image.step * image.height) {
    error_ = "setElevationFromImage: image size, step and data length do not fit";
    ROS_ERROR("TraversabilityMap (MI355X): %s", error_.c_str());
    return false;
  }
  te_image_info info = te_image_info();
  info.height = (int32_t)image.height;
  info.width = (int32_t)image.width;
  info.step = (int32_t)image.step;
  info.channels = layout->second.first;
  info.bytes_per_channel = layout->second.second;
  info.is_bigendian = image.is_bigendian;
  // initializeFromImage: length = resolution * (height, width)
  if (!check(te_set_geometry(ctx_, info.height, info.width, 1, resolution, position.x(), position.y()))) return false;
  if (!check(te_upload_image(ctx_, &info, image.data.data(), TE_LAYER_ELEVATION, 0, (float)minHeight, (float)maxHeight, 0.5))) return false;
  robotSlopeLayer_ = false;
  (void)te_set_layer_present(ctx_, TE_LAYER_ROBOT_SLOPE, 0);  // (as setElevationMap does for a map without the layer)
  geometry_ = grid_map::GridMap();
  grid_map::Length length;
  length(0) = resolution * info.height;
  length(1) = resolution * info.width;
  geometry_.setGeometry(length, resolution, position);
  elevationMapInitialized_ = true;
  elevationFilled_ = elevationSmoothed_ = false;
  traversabilityMapInitialized_ = false;
  footprintLayer_ = polygonLayers_ = false;
  return true;
}

bool TraversabilityMap::moveMap(const grid_map::Position& position, te_move_info& info, const float* const* exposedCells) {
  std::lock_guard<std::mutex> lock(mutex_);
  info = te_move_info();
  if (!ctx_ || !elevationMapInitialized_) {
    error_ = "moveMap: no elevation map";
    ROS_ERROR("Traversability Estimation: Elevation map is not initialized!");
    return false;
  }
  if (fillHoles_ || smoothRadius_ > 0.0) {
    error_ = "moveMap: not with setFillHoles / setSmoothElevation (the strips would enter the elevation layer raw)";
    ROS_ERROR("TraversabilityMap (MI355X): %s", error_.c_str());
    return false;
  }
  if (!check(te_move_map(ctx_, position.x(), position.y(), &info))) return false;
  if (info.n_rects == 0) return true;  // a zero shift: nothing has changed
  const grid_map::Position held = {{info.pos_x, info.pos_y}};
  geometry_.setGeometry(geometry_.getLength(), geometry_.getResolution(), held);
  polygonLayers_ = false;
  const bool computed = traversabilityMapInitialized_, footprint = footprintLayer_;
  // until the loop is through, the map is not one to answer from
  traversabilityMapInitialized_ = footprintLayer_ = false;
  for (int k = 0; k < info.n_rects; ++k) {
    const int32_t* r = info.rects[k];
    if (info.rect_exposed[k] && exposedCells && exposedCells[k] && !check(te_upload_tile(ctx_, exposedCells[k], 0, r[0], r[1], r[2], r[3])))
      return false;
    if (computed && info.results_kept && !check(te_run_chain_region(ctx_, 0, 0, r[0], r[1], r[2], r[3]))) return false;
  }
  if (computed && !info.results_kept && !check(te_run_chain(ctx_, 0))) return false;
  traversabilityMapInitialized_ = computed;
  if (computed && footprint) {
    if (!check(te_run_footprint(ctx_))) return false;
    footprintLayer_ = true;
  }
  return true;
}

bool TraversabilityMap::setFillHoles(const te_median_fill_params* params) {
  std::lock_guard<std::mutex> lock(mutex_);
  if (!params) {
    fillHoles_ = false;
    return true;
  }
  if (!check(te_median_fill_params_validate(params))) return false;
  fillParams_ = *params;
  fillHoles_ = true;
  // (an elevation filled under other parameters stays as it is until the next elevation map: the fill reads its own output)
  return true;
}

bool TraversabilityMap::setSmoothElevation(double radius) {
  std::lock_guard<std::mutex> lock(mutex_);
  if (!(radius >= 0.0) || !std::isfinite(radius)) {
    ROS_ERROR("Traversability Estimation: the smoothing radius must be finite and not negative.");
    return false;
  }
  smoothRadius_ = radius;
  // (an elevation smoothed under another radius stays as it is until the next elevation map: the filter reads its own output)
  return true;
}

bool TraversabilityMap::setNormalsAlgorithm(bool raster) {
  std::lock_guard<std::mutex> lock(mutex_);
  if (!ctx_ || !check(te_set_option(ctx_, TE_OPT_NORMALS_ALGORITHM, raster ? 1 : 0))) return false;
  traversabilityMapInitialized_ = false;  // conservative: computeTraversability() has to run again
  return true;
}

bool TraversabilityMap::computeTraversability() {
  std::lock_guard<std::mutex> lock(mutex_);
  if (!elevationMapInitialized_) {  // :228-231
    ROS_ERROR("Traversability Estimation: Elevation map is not initialized!");
    return false;
  }
  if (fillHoles_ && !elevationFilled_) {
    if (!check(te_run_median_fill(ctx_, &fillParams_, TE_LAYER_ELEVATION, TE_LAYER_ELEVATION, 0, 1))) {
      ROS_ERROR("Traversability Estimation: Could not fill the holes of the elevation map! No traversability computed!");
      traversabilityMapInitialized_ = false;
      return false;
    }
    elevationFilled_ = true;
  }
  if (smoothRadius_ > 0.0 && !elevationSmoothed_) {
    if (!check(te_run_radius_filter(ctx_, TE_RADIUS_MEAN, smoothRadius_, TE_LAYER_ELEVATION, TE_LAYER_ELEVATION, 0, 1))) {
      ROS_ERROR("Traversability Estimation: Could not smooth the elevation map! No traversability computed!");
      traversabilityMapInitialized_ = false;
      return false;
    }
    elevationSmoothed_ = true;
  }
  if (!check(te_run_chain(ctx_, 0))) {  // :214-218
    ROS_ERROR("Traversability Estimation: Could not update the filter chain! No traversability computed!");
    traversabilityMapInitialized_ = false;
    return false;
  }
  traversabilityMapInitialized_ = true;
  footprintLayer_ = polygonLayers_ = false;
  return true;
}

// the circular footprint pass for `radius` (+ the fixed offset of checkCircularFootprintPath); also what marks the
// untraversable cells for the polygon queries
bool TraversabilityMap::ensureCircularFootprint(double radius) {
  if (footprintLayer_ && footprintRadius_ == radius && footprintOffset_ == circularFootprintOffset_) return true;
  te_params p = params_;
  p.fp_radius = radius;
  p.fp_offset = circularFootprintOffset_;
  if (!check(te_set_params(ctx_, &p)) || !check(te_run_footprint(ctx_))) return false;
  params_ = p;
  footprintLayer_ = true;
  footprintRadius_ = radius;
  footprintOffset_ = circularFootprintOffset_;
  return true;
}

bool TraversabilityMap::traversabilityFootprint(const double& radius, const double& offset) {
  std::lock_guard<std::mutex> lock(mutex_);
  if (!traversabilityMapInitialized_) return false;  // :308
  te_params p = params_;
  p.fp_radius = radius;
  p.fp_offset = offset;
  if (!check(te_set_params(ctx_, &p)) || !check(te_run_footprint(ctx_))) return false;
  params_ = p;
  footprintLayer_ = true;
  footprintRadius_ = radius;
  footprintOffset_ = offset;
  return true;
}

bool TraversabilityMap::traversabilityFootprint(double footprintYaw) {
  std::lock_guard<std::mutex> lock(mutex_);
  if (!traversabilityMapInitialized_) return false;  // :240
  if (footprintPoints_.empty()) {
    error_ = "no footprint polygon set (footprint/footprint_polygon)";
    ROS_ERROR("TraversabilityMap (MI355X): %s", error_.c_str());
    return false;
  }
  if (!footprintLayer_ && !ensureCircularFootprint(params_.fp_radius)) return false;  // marks the untraversable cells
  std::vector<double> xy;
  for (const geometry_msgs::Point32& pt : footprintPoints_) {  // :273-276 float -> double
    xy.push_back(pt.x);
    xy.push_back(pt.y);
  }
  if (!check(te_run_polygon_footprint(ctx_, (int)footprintPoints_.size(), xy.data(), footprintYaw))) return false;
  polygonLayers_ = true;
  return true;
}

bool TraversabilityMap::checkFootprintPath(const traversability_msgs::FootprintPath& path,
                                           traversability_msgs::TraversabilityResult& result) {
  std::vector<traversability_msgs::TraversabilityResult> results;
  const bool ok = checkFootprintPaths(std::vector<traversability_msgs::FootprintPath>(1, path), results);
  if (!results.empty())
    result = results[0];
  else
    result.is_safe = static_cast<unsigned char>(false);
  return ok;
}

bool TraversabilityMap::checkFootprintPaths(const std::vector<traversability_msgs::FootprintPath>& paths,
                                            std::vector<traversability_msgs::TraversabilityResult>& results) {
  std::lock_guard<std::mutex> lock(mutex_);
  results.clear();
  if (paths.empty()) {
    ROS_WARN("No footprint path available to check!");  // TraversabilityEstimation.cpp:281-284
    return false;
  }
  // the service stops at the first path without poses (:330-334 -> TraversabilityEstimation.cpp:290)
  size_t n = paths.size();
  bool complete = true;
  for (size_t k = 0; k < paths.size(); ++k)
    if (paths[k].poses.poses.empty()) {
      ROS_WARN("Traversability Estimation: This path has no poses to check!");
      n = k;
      complete = false;
      break;
    }
  results.assign(n, traversability_msgs::TraversabilityResult());
  if (!traversabilityMapInitialized_) {  // :323-327
    ROS_WARN("Traversability Estimation: check Footprint path: Traversability map not yet initialized.");
    return complete;
  }
  // polygonal footprints: one batch per distinct footprint; circular ones: one batch per distinct radius
  std::map<double, std::vector<size_t>> circular;
  std::vector<size_t> polygonal;
  for (size_t k = 0; k < n; ++k) {
    if (paths[k].footprint.polygon.points.empty())
      circular[paths[k].radius].push_back(k);
    else
      polygonal.push_back(k);
  }
  std::vector<bool> done(n, false);
  for (size_t a = 0; a < polygonal.size(); ++a) {
    const size_t lead = polygonal[a];
    if (done[lead]) continue;
    const std::vector<geometry_msgs::Point32>& pts = paths[lead].footprint.polygon.points;
    std::vector<size_t> group;
    for (size_t b = a; b < polygonal.size(); ++b) {
      const std::vector<geometry_msgs::Point32>& q = paths[polygonal[b]].footprint.polygon.points;
      bool same = !done[polygonal[b]] && q.size() == pts.size();
      for (size_t m = 0; same && m < q.size(); ++m) same = q[m].x == pts[m].x && q[m].y == pts[m].y && q[m].z == pts[m].z;
      if (same) group.push_back(polygonal[b]);
    }
    if (!footprintLayer_ && !ensureCircularFootprint(params_.fp_radius)) return false;
    std::vector<int> offset(1, 0);
    std::vector<double> poses, points;
    std::vector<unsigned char> conservative;
    for (const geometry_msgs::Point32& pt : pts) {  // :502-504 float -> double
      points.push_back(pt.x);
      points.push_back(pt.y);
      points.push_back(pt.z);
    }
    for (size_t k : group) {
      for (const geometry_msgs::Pose& pose : paths[k].poses.poses) {
        const double v[7] = {pose.position.x,    pose.position.y,    pose.position.z,   pose.orientation.x,
                             pose.orientation.y, pose.orientation.z, pose.orientation.w};
        poses.insert(poses.end(), v, v + 7);
      }
      offset.push_back((int)(poses.size() / 7));
      conservative.push_back(paths[k].conservative);
      done[k] = true;
    }
    std::vector<unsigned char> safe(group.size());
    std::vector<double> trav(group.size()), area(group.size());
    std::vector<int> status(group.size());
    if (!check(te_check_polygon_footprint_paths(ctx_, 0, (int)group.size(), offset.data(), poses.data(), (int)pts.size(),
                                                points.data(), conservative.data(), safe.data(), trav.data(), area.data(),
                                                status.data())))
      return false;
    for (size_t m = 0; m < group.size(); ++m) {
      results[group[m]].is_safe = safe[m];
      results[group[m]].traversability = trav[m];
      results[group[m]].area = area[m];
    }
  }
  if (pathCheckOnDemand_ && !circular.empty()) {
    // every circular path of the request in one call, each at its own path.radius, evaluated on demand at the centres it
    // visits: no footprint pass, and footprintLayer_, footprintRadius_ and params_ stay as they are
    std::vector<size_t> group;
    for (size_t k = 0; k < n; ++k)
      if (paths[k].footprint.polygon.points.empty()) group.push_back(k);
    std::vector<int> offset(1, 0);
    std::vector<double> xy, radius;
    for (size_t k : group) {
      for (const geometry_msgs::Pose& pose : paths[k].poses.poses) {
        xy.push_back(pose.position.x);
        xy.push_back(pose.position.y);
      }
      offset.push_back((int)(xy.size() / 2));
      radius.push_back(paths[k].radius);
    }
    std::vector<unsigned char> safe(group.size());
    std::vector<double> trav(group.size());
    std::vector<int> status(group.size());
    if (!check(te_check_footprint_paths_radius(ctx_, 0, (int)group.size(), offset.data(), xy.data(), radius.data(),
                                               circularFootprintOffset_, safe.data(), trav.data(), status.data(), nullptr)))
      return false;
    for (size_t m = 0; m < group.size(); ++m) {
      results[group[m]].is_safe = safe[m];
      results[group[m]].traversability = trav[m];
      results[group[m]].area = 0.0;  // :355: never set for circular footprints
    }
    return complete;
  }
  for (const auto& entry : circular) {
    if (!ensureCircularFootprint(entry.first)) return false;
    const std::vector<size_t>& group = entry.second;
    std::vector<int> offset(1, 0);
    std::vector<double> xy;
    for (size_t k : group) {
      for (const geometry_msgs::Pose& pose : paths[k].poses.poses) {
        xy.push_back(pose.position.x);
        xy.push_back(pose.position.y);
      }
      offset.push_back((int)(xy.size() / 2));
    }
    std::vector<unsigned char> safe(group.size());
    std::vector<double> trav(group.size());
    std::vector<int> status(group.size());
    if (!check(te_check_footprint_paths(ctx_, 0, (int)group.size(), offset.data(), xy.data(), safe.data(), trav.data(),
                                        status.data())))
      return false;
    for (size_t m = 0; m < group.size(); ++m) {
      results[group[m]].is_safe = safe[m];
      results[group[m]].traversability = trav[m];
      results[group[m]].area = 0.0;  // :355: never set for circular footprints
    }
  }
  return complete;
}

int TraversabilityMap::deviceLayer(const std::string& name) const {
  if (!elevationMapInitialized_) return -1;
  if (name == "elevation") return TE_LAYER_ELEVATION;
  if (traversabilityMapInitialized_) {
    if (name == "traversability_slope") return TE_LAYER_SLOPE;
    if (name == "traversability_step") return TE_LAYER_STEP;
    if (name == "traversability_roughness") return TE_LAYER_ROUGHNESS;
    if (name == "traversability") return TE_LAYER_TRAVERSABILITY;
  }
  if (footprintLayer_ && name == "traversability_footprint") return TE_LAYER_FOOTPRINT;
  if (polygonLayers_ && name == "traversability_x") return TE_LAYER_TRAVERSABILITY_X;
  if (polygonLayers_ && name == "traversability_rot") return TE_LAYER_TRAVERSABILITY_ROT;
  return -1;
}

bool TraversabilityMap::getOccupancyGrid(const std::string& layer, float dataMin, float dataMax, nav_msgs::OccupancyGrid& grid) {
  std::lock_guard<std::mutex> lock(mutex_);
  const int id = deviceLayer(layer);
  if (!ctx_ || id < 0) {
    error_ = "getOccupancyGrid: no layer '" + layer + "'";
    return false;
  }
  const int rows = geometry_.getSize()(0), cols = geometry_.getSize()(1);
  grid.data.resize((size_t)rows * cols);
  if (!check(te_download_occupancy(ctx_, 0, 1, &id, &dataMin, &dataMax, grid.data.data()))) return false;
  // (toOccupancyGrid: the device layers are in logical order, so the start index does not enter)
  grid.info.map_load_time = grid.header.stamp;  // (toOccupancyGrid: the header's stamp, which the caller has set)
  grid.info.resolution = (float)geometry_.getResolution();
  grid.info.width = (uint32_t)rows;
  grid.info.height = (uint32_t)cols;
  grid.info.origin = geometry_msgs::Pose();
  grid.info.origin.position.x = geometry_.getPosition().x() - 0.5 * geometry_.getLength().x();
  grid.info.origin.position.y = geometry_.getPosition().y() - 0.5 * geometry_.getLength().y();
  return true;
}

bool TraversabilityMap::getPointCloud(const std::vector<std::string>& layers, const std::string& pointLayer, sensor_msgs::PointCloud2& cloud) {
  std::lock_guard<std::mutex> lock(mutex_);
  std::vector<int> ids;
  const int point = deviceLayer(pointLayer);
  for (const std::string& name : layers) ids.push_back(deviceLayer(name));
  for (size_t k = 0; k < ids.size(); ++k)
    if (ids[k] < 0) {
      error_ = "getPointCloud: no layer '" + layers[k] + "'";
      return false;
    }
  if (!ctx_ || point < 0 || ids.empty()) {
    error_ = "getPointCloud: no point layer '" + pointLayer + "'";
    return false;
  }
  // one call -- count, scan, scatter, one transfer of the points found -- into room for every cell; the rest is given back
  size_t n = 0;
  const size_t cells = (size_t)geometry_.getSize()(0) * geometry_.getSize()(1);
  const uint32_t nFields = (uint32_t)ids.size() + 2;
  cloud.data.resize(cells * nFields * sizeof(float));
  if (!check(te_download_cloud(ctx_, 0, (int)ids.size(), ids.data(), point, 0, nullptr, reinterpret_cast<float*>(cloud.data.data()), cells, &n))) {
    cloud.data.clear();
    return false;
  }
  cloud.data.resize(n * nFields * sizeof(float));
  cloud.fields.clear();
  for (size_t k = 0; k < ids.size(); ++k)
    for (const std::string& name : ids[k] == point ? std::vector<std::string>{"x", "y", "z"} : std::vector<std::string>{layers[k]}) {
      sensor_msgs::PointField f;
      f.name = name;
      f.offset = (uint32_t)(4 * cloud.fields.size());
      f.datatype = sensor_msgs::PointField::FLOAT32;
      f.count = 1;
      cloud.fields.push_back(f);
    }
  cloud.height = 1;
  cloud.width = (uint32_t)n;
  cloud.is_bigendian = 0;
  cloud.point_step = 4 * nFields;
  cloud.row_step = cloud.width * cloud.point_step;
  cloud.is_dense = 0;
  return true;
}

bool TraversabilityMap::getTraversabilityMap(const grid_map::Position& position, const grid_map::Length& length,
                                             const std::vector<std::string>& layers, std::vector<uint8_t>& message, const te_msg_info* header) {
  std::lock_guard<std::mutex> lock(mutex_);
  message.clear();
  error_.clear();
  std::vector<std::string> names = layers;
  if (names.empty())  // (:306-307: toMessage(subMap, response.map) takes every layer)
    for (const char* name : {"elevation", "traversability_slope", "traversability_step", "traversability_roughness", "traversability",
                             "traversability_footprint", "traversability_x", "traversability_rot"})
      if (deviceLayer(name) >= 0) names.push_back(name);
  std::vector<int> ids;
  std::vector<const char*> cnames;
  for (const std::string& name : names) {
    ids.push_back(deviceLayer(name));
    cnames.push_back(name.c_str());
    if (ids.back() < 0) {
      error_ = "getTraversabilityMap: no layer '" + name + "'";
      return false;
    }
  }
  if (!ctx_ || ids.empty()) {
    error_ = "getTraversabilityMap: no map";
    return false;
  }
  te_msg_info info = header ? *header : te_msg_info();
  if (!header) info.pose[6] = 1.0;
  te_submap_info sub;
  size_t need = 0;
  // the sizing call runs the geometry only: it reports the size with TE_ERR_INVALID_ARG (no room), and TE_OK without a size
  // for a request getSubmap refuses (sub.ok == 0, the service's isSuccess = false)
  const int rc = te_download_submap_msg(ctx_, &info, position.x(), position.y(), length.x(), length.y(), (int)ids.size(), ids.data(),
                                        cnames.data(), 0, nullptr, &sub, nullptr, 0, &need);
  if (need == 0) return rc == TE_OK ? false : check(rc);
  message.resize(need);
  if (!check(te_download_submap_msg(ctx_, &info, position.x(), position.y(), length.x(), length.y(), (int)ids.size(), ids.data(), cnames.data(), 0,
                                    nullptr, &sub, message.data(), message.size(), &need)) ||
      !sub.ok) {
    message.clear();
    return false;
  }
  message.resize(need);
  return true;
}

grid_map::GridMap TraversabilityMap::getTraversabilityMap() {
  std::lock_guard<std::mutex> lock(mutex_);
  grid_map::GridMap map = geometry_;
  if (!elevationMapInitialized_) return map;
  struct Entry {
    const char* name;
    int layer;
    bool present;
  };
  const Entry entries[] = {{"elevation", TE_LAYER_ELEVATION, true},
                           {"traversability_slope", TE_LAYER_SLOPE, traversabilityMapInitialized_},
                           {"traversability_step", TE_LAYER_STEP, traversabilityMapInitialized_},
                           {"traversability_roughness", TE_LAYER_ROUGHNESS, traversabilityMapInitialized_},
                           {"traversability", TE_LAYER_TRAVERSABILITY, traversabilityMapInitialized_},
                           {"traversability_footprint", TE_LAYER_FOOTPRINT, footprintLayer_},
                           {"traversability_x", TE_LAYER_TRAVERSABILITY_X, polygonLayers_},
                           {"traversability_rot", TE_LAYER_TRAVERSABILITY_ROT, polygonLayers_}};
  const auto start = map.getStartIndex();
  for (const Entry& e : entries) {
    if (!e.present) continue;
    map.add(e.name);
    if (!check(te_download_layer_circular(ctx_, e.layer, map.get(e.name).data(), 0, start(0), start(1)))) map.erase(e.name);
  }
  return map;
}

}  // namespace traversability_estimation_gpu
