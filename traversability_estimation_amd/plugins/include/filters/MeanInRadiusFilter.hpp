/*
 * MeanInRadiusFilter.hpp -- traversabilityFilters/MeanInRadiusFilter on MI355X: gridMapFilters/MeanInRadiusFilter (grid_map_filters),
 * the radial blur a grid_map pipeline puts between the hole filling and the normals, computed on the device
 * (te_run_radius_filter).  New and optional; it reads the upstream filter's parameter keys, so that entry of the YAML can be
 * pointed here by changing its `type:` line only.  The contract -- restated from memory, grid_map_filters is not in the
 * reference tree -- is in include/travgpu.h.  InRadiusFilter is what this filter and MinInRadiusFilter share.
 */
#ifndef TRAVGPU_MEANINRADIUSFILTER_HPP
#define TRAVGPU_MEANINRADIUSFILTER_HPP

#include <filters/filter_base.h>
#include <string>

#include "travgpu.h"

namespace filters {

template <typename T>
class InRadiusFilter : public FilterBase<T> {
 public:
  /*! op: TE_RADIUS_MEAN / TE_RADIUS_MIN; name: the filter's name in messages. */
  InRadiusFilter(int op, const char* name);
  virtual ~InRadiusFilter();
  /*! Keys of the upstream filters, all required: radius (finite, >= 0; 0 is the centre cell alone), input_layer, output_layer. */
  virtual bool configure();
  /*! mapOut = mapIn with output_layer = the mean / minimum of input_layer within radius.  The input goes into the device's
   *  elevation layer and is filtered in place there, so the plugins behind this one that read output_layer as their elevation
   *  find it resident. */
  virtual bool update(const T& mapIn, T& mapOut);

 private:
  int op_;
  std::string name_;
  double radius_;
  std::string inputLayer_, outputLayer_;
};

template <typename T>
class MeanInRadiusFilter : public InRadiusFilter<T> {
 public:
  MeanInRadiusFilter() : InRadiusFilter<T>(TE_RADIUS_MEAN, "MeanInRadius filter") {}
};

}  // namespace filters
#endif
