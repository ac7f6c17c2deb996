/* MinInRadiusFilter.cpp -- see include/filters/MinInRadiusFilter.hpp; the shared members: MeanInRadiusFilter.cpp */
#include "filters/MinInRadiusFilter.hpp"

#include <pluginlib/class_list_macros.h>
#include <grid_map_ros/grid_map_ros.hpp>

namespace filters {
extern template class InRadiusFilter<grid_map::GridMap>;
}

PLUGINLIB_EXPORT_CLASS(filters::MinInRadiusFilter<grid_map::GridMap>, filters::FilterBase<grid_map::GridMap>)
