/* MedianFillFilter.cpp -- see include/filters/MedianFillFilter.hpp */
#include "filters/MedianFillFilter.hpp"

#include <mutex>

#include <pluginlib/class_list_macros.h>
#include <grid_map_ros/grid_map_ros.hpp>

#include "travgpu_plugins/DeviceMap.hpp"

using travgpu_plugins::DeviceMap;

namespace filters {

template <typename T>
MedianFillFilter<T>::MedianFillFilter() {
  te_median_fill_params_default(&params_);
}

template <typename T>
MedianFillFilter<T>::~MedianFillFilter() {}

template <typename T>
bool MedianFillFilter<T>::configure() {
  if (!FilterBase<T>::getParam(std::string("input_layer"), inputLayer_)) {
    ROS_ERROR("Median fill filter did not find parameter `input_layer`.");
    return false;
  }
  if (!FilterBase<T>::getParam(std::string("output_layer"), outputLayer_)) {
    ROS_ERROR("Median fill filter did not find parameter `output_layer`.");
    return false;
  }
  te_median_fill_params_default(&params_);
  FilterBase<T>::getParam(std::string("fill_hole_radius"), params_.fill_hole_radius);
  FilterBase<T>::getParam(std::string("existing_value_radius"), params_.existing_value_radius);
  bool filterExisting = false;
  FilterBase<T>::getParam(std::string("filter_existing_values"), filterExisting);
  params_.filter_existing_values = filterExisting ? 1 : 0;
  int iterations = params_.num_erode_dilation_iterations;
  FilterBase<T>::getParam(std::string("num_erode_dilation_iterations"), iterations);
  params_.num_erode_dilation_iterations = iterations;
  std::string maskLayer;
  bool debug = false;
  if (FilterBase<T>::getParam(std::string("fill_mask_layer"), maskLayer))
    ROS_DEBUG("MedianFillFilter (MI355X): fill_mask_layer '%s' is ignored, every update computes its mask", maskLayer.c_str());
  if (FilterBase<T>::getParam(std::string("debug"), debug) && debug) ROS_DEBUG("MedianFillFilter (MI355X): the debug layers are not built");
  if (te_median_fill_params_validate(&params_) != TE_OK) {
    ROS_ERROR("%s", te_last_error());
    return false;
  }
  return true;
}

template <typename T>
bool MedianFillFilter<T>::update(const T& mapIn, T& mapOut) {
  mapOut = mapIn;
  if (!mapOut.exists(inputLayer_)) {
    ROS_ERROR("Check your layer type! Type %s does not exist", inputLayer_.c_str());
    return false;
  }
  DeviceMap& dev = DeviceMap::instance();
  std::lock_guard<std::mutex> lock(dev.mutex());
  const bool ok = dev.filterElevation(mapOut, inputLayer_, outputLayer_, [&] { return dev.runMedianFill(params_, TE_LAYER_ELEVATION, TE_LAYER_ELEVATION); });
  if (!ok) ROS_ERROR("MedianFillFilter (MI355X): %s", dev.error().c_str());
  return ok;
}

}  // namespace filters

PLUGINLIB_EXPORT_CLASS(filters::MedianFillFilter<grid_map::GridMap>, filters::FilterBase<grid_map::GridMap>)
