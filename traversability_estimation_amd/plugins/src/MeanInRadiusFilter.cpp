/* MeanInRadiusFilter.cpp -- see include/filters/MeanInRadiusFilter.hpp */
#include "filters/MeanInRadiusFilter.hpp"

#include <cmath>
#include <mutex>

#include <pluginlib/class_list_macros.h>
#include <grid_map_ros/grid_map_ros.hpp>

#include "travgpu_plugins/DeviceMap.hpp"

using travgpu_plugins::DeviceMap;

namespace filters {

template <typename T>
InRadiusFilter<T>::InRadiusFilter(int op, const char* name) : op_(op), name_(name), radius_(0.0) {}

template <typename T>
InRadiusFilter<T>::~InRadiusFilter() {}

template <typename T>
bool InRadiusFilter<T>::configure() {
  if (!FilterBase<T>::getParam(std::string("radius"), radius_)) {
    ROS_ERROR("%s did not find parameter `radius`.", name_.c_str());
    return false;
  }
  if (!(radius_ >= 0.0) || !std::isfinite(radius_)) {
    ROS_ERROR("%s: radius must be finite and not negative.", name_.c_str());
    return false;
  }
  if (!FilterBase<T>::getParam(std::string("input_layer"), inputLayer_)) {
    ROS_ERROR("%s did not find parameter `input_layer`.", name_.c_str());
    return false;
  }
  if (!FilterBase<T>::getParam(std::string("output_layer"), outputLayer_)) {
    ROS_ERROR("%s did not find parameter `output_layer`.", name_.c_str());
    return false;
  }
  return true;
}

template <typename T>
bool InRadiusFilter<T>::update(const T& mapIn, T& mapOut) {
  mapOut = mapIn;
  if (!mapOut.exists(inputLayer_)) {
    ROS_ERROR("Check your layer type! Type %s does not exist", inputLayer_.c_str());
    return false;
  }
  DeviceMap& dev = DeviceMap::instance();
  std::lock_guard<std::mutex> lock(dev.mutex());
  const bool ok = dev.filterElevation(mapOut, inputLayer_, outputLayer_, [&] { return dev.runRadiusFilter(op_, radius_, TE_LAYER_ELEVATION, TE_LAYER_ELEVATION); });
  if (!ok) ROS_ERROR("%s (MI355X): %s", name_.c_str(), dev.error().c_str());
  return ok;
}

template class InRadiusFilter<grid_map::GridMap>;

}  // namespace filters

PLUGINLIB_EXPORT_CLASS(filters::MeanInRadiusFilter<grid_map::GridMap>, filters::FilterBase<grid_map::GridMap>)
