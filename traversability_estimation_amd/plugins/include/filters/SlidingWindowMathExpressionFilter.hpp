/*
 * SlidingWindowMathExpressionFilter.hpp -- traversabilityFilters/SlidingWindowMathExpressionFilter on MI355X:
 * gridMapFilters/SlidingWindowMathExpressionFilter (grid_map_filters), an EigenLab expression over a square window around every
 * cell -- a local standard deviation, a box mean, a local relief -- computed on the device (te_run_window_expression).  New and
 * optional; it reads the upstream filter's parameter keys, so that entry of the YAML can be pointed here by changing its
 * `type:` line only.  The contract -- restated from memory, grid_map_filters and EigenLab are not in the reference tree -- is in
 * include/travgpu.h.
 */
#ifndef TRAVGPU_SLIDINGWINDOWMATHEXPRESSIONFILTER_HPP
#define TRAVGPU_SLIDINGWINDOWMATHEXPRESSIONFILTER_HPP

#include <filters/filter_base.h>
#include <string>

#include "travgpu.h"

namespace filters {

template <typename T>
class SlidingWindowMathExpressionFilter : public FilterBase<T> {
 public:
  SlidingWindowMathExpressionFilter();
  virtual ~SlidingWindowMathExpressionFilter();
  /*! Keys of the upstream filter: input_layer, output_layer, expression (required); exactly one of window_size (odd, >= 1)
   *  and window_length (metres, finite, >= 0); compute_empty_cells (default true); edge_handling (inside | crop | empty |
   *  mean, default inside).  The expression is compiled here (te_window_expr_check): one that the device would refuse is
   *  refused now, with the column in the message. */
  virtual bool configure();
  /*! mapOut = mapIn with output_layer = the expression over the window of every cell of input_layer.  The input goes into the
   *  device's elevation layer (the plugins behind this one that read it find it resident), the result is written beside it. */
  virtual bool update(const T& mapIn, T& mapOut);

 private:
  std::string inputLayer_, outputLayer_, expression_;
  std::string deviceExpression_;  // expression_ with input_layer written as the device layer's own name
  te_window_expr_params params_;
};

}  // namespace filters
#endif
