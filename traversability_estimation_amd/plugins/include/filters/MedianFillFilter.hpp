/*
 * MedianFillFilter.hpp -- traversabilityFilters/MedianFillFilter on MI355X: gridMapFilters/MedianFillFilter (grid_map_filters),
 * the hole filling a grid_map pipeline puts in front of the traversability chain, computed on the device (te_run_median_fill).
 * New and optional; it reads the upstream filter's parameter keys, so that entry of the YAML can be pointed here by changing
 * its `type:` line only.  The contract -- restated from memory, grid_map_filters is not in the reference tree -- is in
 * include/travgpu.h.
 */
#ifndef TRAVGPU_MEDIANFILLFILTER_HPP
#define TRAVGPU_MEDIANFILLFILTER_HPP

#include <filters/filter_base.h>
#include <string>

#include "travgpu.h"

namespace filters {

template <typename T>
class MedianFillFilter : public FilterBase<T> {
 public:
  MedianFillFilter();
  virtual ~MedianFillFilter();
  /*! Keys of the upstream filter: input_layer and output_layer (required), fill_hole_radius (0.05), filter_existing_values
   *  (false), existing_value_radius (0.0), num_erode_dilation_iterations (4).  fill_mask_layer and debug are accepted and
   *  ignored: every update computes its mask afresh, and the debug layers are not built. */
  virtual bool configure();
  /*! mapOut = mapIn with output_layer = the filled input_layer.  When the input is the chain's elevation the filled layer stays
   *  resident on the device: the plugins behind this one that read output_layer as their elevation find it there. */
  virtual bool update(const T& mapIn, T& mapOut);

 private:
  te_median_fill_params params_;
  std::string inputLayer_, outputLayer_;
};

}  // namespace filters
#endif
