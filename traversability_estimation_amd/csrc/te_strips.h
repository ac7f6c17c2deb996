// te_strips.h -- how many rows a strip of a marching launch takes.  Plain C++: the step kernels' launchers (te_step5.hip),
// the footprint route (te_fp_route.h) and its CPU check compile the same text.
#pragma once

namespace te {
namespace fast {

// Rows per strip such that (column blocks x maps x strips) fills `slots` resident waves in one round (at least 1 row;
// more than max_rows per strip gains nothing and keeps short maps from waiting on one long strip)
inline int plan_strip_rows(int rows, long columns, long slots, int max_rows = 512) {
  long strips = slots / (columns > 0 ? columns : 1);
  if (strips < 1) strips = 1;
  long per = (rows + strips - 1) / strips;
  if (per > max_rows) per = max_rows;
  if (per < 1) per = 1;
  return (int)per;
}

}  // namespace fast
}  // namespace te
