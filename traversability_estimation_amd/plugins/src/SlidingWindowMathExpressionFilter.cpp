/* SlidingWindowMathExpressionFilter.cpp -- see include/filters/SlidingWindowMathExpressionFilter.hpp */
#include "filters/SlidingWindowMathExpressionFilter.hpp"

#include <cctype>
#include <cmath>
#include <mutex>

#include <pluginlib/class_list_macros.h>
#include <grid_map_ros/grid_map_ros.hpp>

#include "travgpu_plugins/DeviceMap.hpp"

using travgpu_plugins::DeviceMap;

namespace filters {

namespace {

const char* const kDeviceLayer = "elevation";  // the name of TE_LAYER_ELEVATION in an expression

// `text` with every identifier equal to `from` written as `to` (whole identifiers only: a function name is never a layer)
std::string rename_identifier(const std::string& text, const std::string& from, const std::string& to) {
  std::string out;
  for (size_t k = 0; k < text.size();) {
    const unsigned char ch = (unsigned char)text[k];
    if (std::isalpha(ch) || ch == '_') {
      size_t e = k;
      while (e < text.size() && (std::isalnum((unsigned char)text[e]) || text[e] == '_')) ++e;
      const std::string word = text.substr(k, e - k);
      out += word == from ? to : word;
      k = e;
    } else {
      out += text[k++];
    }
  }
  return out;
}

}  // namespace

template <typename T>
SlidingWindowMathExpressionFilter<T>::SlidingWindowMathExpressionFilter() {
  te_window_expr_params_default(&params_);
}

template <typename T>
SlidingWindowMathExpressionFilter<T>::~SlidingWindowMathExpressionFilter() {}

template <typename T>
bool SlidingWindowMathExpressionFilter<T>::configure() {
  const char* name = "SlidingWindowMathExpressionFilter";
  if (!FilterBase<T>::getParam(std::string("input_layer"), inputLayer_)) {
    ROS_ERROR("%s did not find parameter 'input_layer'.", name);
    return false;
  }
  if (!FilterBase<T>::getParam(std::string("output_layer"), outputLayer_)) {
    ROS_ERROR("%s did not find parameter 'output_layer'.", name);
    return false;
  }
  if (!FilterBase<T>::getParam(std::string("expression"), expression_)) {
    ROS_ERROR("%s did not find parameter 'expression'.", name);
    return false;
  }
  te_window_expr_params_default(&params_);
  int windowSize = 0;
  double windowLength = 0.0;
  const bool haveSize = FilterBase<T>::getParam(std::string("window_size"), windowSize);
  const bool haveLength = FilterBase<T>::getParam(std::string("window_length"), windowLength);
  if (haveSize == haveLength) {
    ROS_ERROR("%s needs exactly one of 'window_size' and 'window_length'.", name);
    return false;
  }
  params_.window_size = haveSize ? windowSize : 0;
  params_.use_window_length = haveLength ? 1 : 0;
  params_.window_length = haveLength ? windowLength : 0.0;
  bool computeEmptyCells = true;
  FilterBase<T>::getParam(std::string("compute_empty_cells"), computeEmptyCells);
  params_.compute_empty_cells = computeEmptyCells ? 1 : 0;
  std::string edge = "inside";
  FilterBase<T>::getParam(std::string("edge_handling"), edge);
  if (edge == "inside") {
    params_.edge_handling = TE_EDGE_INSIDE;
  } else if (edge == "crop") {
    params_.edge_handling = TE_EDGE_CROP;
  } else if (edge == "empty") {
    params_.edge_handling = TE_EDGE_EMPTY;
  } else if (edge == "mean") {
    params_.edge_handling = TE_EDGE_MEAN;
  } else {
    ROS_ERROR("%s: 'edge_handling' must be one of inside, crop, empty, mean.", name);
    return false;
  }
  if (te_window_expr_params_validate(&params_) != TE_OK) {
    ROS_ERROR("%s: %s", name, te_last_error());
    return false;
  }
  // the device layer has its own name: an identifier that already is that name and is not the input layer would be mistaken for it
  if (inputLayer_ != kDeviceLayer && rename_identifier(expression_, kDeviceLayer, "") != expression_) {
    ROS_ERROR("%s: the expression names '%s', which is not the input layer.", name, kDeviceLayer);
    return false;
  }
  deviceExpression_ = rename_identifier(expression_, inputLayer_, kDeviceLayer);
  if (te_window_expr_check(deviceExpression_.c_str(), TE_LAYER_ELEVATION, nullptr) != TE_OK) {
    ROS_ERROR("%s: %s", name, te_last_error());
    return false;
  }
  return true;
}

template <typename T>
bool SlidingWindowMathExpressionFilter<T>::update(const T& mapIn, T& mapOut) {
  mapOut = mapIn;
  if (!mapOut.exists(inputLayer_)) {
    ROS_ERROR("Check your layer type! Type %s does not exist", inputLayer_.c_str());
    return false;
  }
  DeviceMap& dev = DeviceMap::instance();
  std::lock_guard<std::mutex> lock(dev.mutex());
  // the window of length window_length is taken at the map's own resolution, by the library
  const int outSlot = TE_LAYER_ROUGHNESS;  // a float layer beside the input: the result leaves through it
  bool ok = dev.prepare(mapOut) && dev.upload(mapOut, inputLayer_, TE_LAYER_ELEVATION) &&
            dev.runWindowExpression(params_, deviceExpression_, TE_LAYER_ELEVATION, outSlot);
  if (ok) {
    if (!mapOut.exists(outputLayer_)) mapOut.add(outputLayer_);
    ok = dev.download(mapOut, outputLayer_, outSlot);
  }
  if (!ok) ROS_ERROR("SlidingWindowMathExpressionFilter (MI355X): %s", dev.error().c_str());
  return ok;
}

template class SlidingWindowMathExpressionFilter<grid_map::GridMap>;

}  // namespace filters

PLUGINLIB_EXPORT_CLASS(filters::SlidingWindowMathExpressionFilter<grid_map::GridMap>, filters::FilterBase<grid_map::GridMap>)
