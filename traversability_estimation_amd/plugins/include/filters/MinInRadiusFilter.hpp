/*
 * MinInRadiusFilter.hpp -- traversabilityFilters/MinInRadiusFilter on MI355X: gridMapFilters/MinInRadiusFilter (grid_map_filters),
 * the conservative lower surface, computed on the device (te_run_radius_filter).  New and optional; the upstream filter's keys
 * (MeanInRadiusFilter.hpp: InRadiusFilter).  The contract is in include/travgpu.h.
 */
#ifndef TRAVGPU_MININRADIUSFILTER_HPP
#define TRAVGPU_MININRADIUSFILTER_HPP

#include "filters/MeanInRadiusFilter.hpp"

namespace filters {

template <typename T>
class MinInRadiusFilter : public InRadiusFilter<T> {
 public:
  MinInRadiusFilter() : InRadiusFilter<T>(TE_RADIUS_MIN, "MinInRadius filter") {}
};

}  // namespace filters
#endif
