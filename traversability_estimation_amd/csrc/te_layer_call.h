// te_layer_call.h -- the call contract of the layer filters: which layer a call may read, which it may write, which maps of the
// batch and which rectangle it may name, and whether it runs in place.  Plain C++, no HIP: the CPU test
// (tests/cpu/layer_call_check.cpp) holds it to the rules restated as a table.  It is the only statement of these rules: the
// entry points fill Facts from their context (te_ctx.h: facts_of), call one of the forms below and turn a refusal into their
// status and message (te_ctx.h: refused):
//   check                        te_run_median_fill, te_run_radius_filter, te_run_window_expression, their te_time_*_samples,
//                                te_copy_layer
//   check_region                 te_run_median_fill_region, te_run_radius_filter_region, te_run_window_expression_region
//   check_update(_region)        te_run_threshold(_region): one layer read and rewritten in place
//   check_expression_operand,    te_run_expression(_region), te_run_layer_expression(_thresholds)(_region): each layer the text
//   check_expression_output      reads, and the layer it writes
//
// A layer can be read when it has memory and holds values: the elevation once one was uploaded, robot_slope once it was
// written, the layers only some runs write (kOptional) once a run or an upload wrote them -- the two polygon layers as soon
// as they have memory, which only te_run_polygon_footprint gives them.  Every layer with memory can be written, and
// robot_slope always: it gets its memory from its first write.
//
// User layers (te_user_layers.h: ids TE_LAYER_COUNT .. TE_LAYER_COUNT + 15): one that was added is a layer like any other -- read
// once it has memory and was written (layers_written), written always, its memory coming from the first write as robot_slope's
// does.  An id that was never added is refused exactly as an id out of range is.
#pragma once
#include "te_ctx_state.h"
#include "te_region_plan.h"

namespace te {
namespace layer_call {

// what the decision rests on
struct Facts {
  bool have_geo = false;
  int batch = 0, rows = 0, cols = 0;
  unsigned has_memory = 0;      // bit TE_LAYER_* of every layer with device memory
  unsigned layers_written = 0;  // CtxState::layers_written()
  bool have_robot_slope = false, have_elev = false;  // CtxState::have_robot_slope(), have_elev()
  unsigned user_added = 0;      // bit id of every user layer that was added (user::Table::mask())
};

// the rules in the order they are tried: the first that fails is the verdict
enum Rule {
  kAccepted = 0, kNoGeometry, kBadOutput, kBadMaps, kTooManyMaps, kBadInput, kInputAbsent, kOutputNoMemory,
  // of the region forms: the one map, in_layer == out_layer, the rectangle
  kBadMap, kRegionInPlace, kBadRect,
  // of an expression: a layer its text reads
  kOperandAbsent
};

struct Verdict {
  int code;       // the status the entry point returns
  Rule rule;
  int id;         // the layer id kBadOutput, kBadInput, kInputAbsent, kOutputNoMemory, kRegionInPlace or kOperandAbsent refused; -1 otherwise
  bool in_place;  // accepted, and in_layer == out_layer: the kernels must read a copy
};

constexpr unsigned kPolygonLayers = layer_bit(TE_LAYER_TRAVERSABILITY_X) | layer_bit(TE_LAYER_TRAVERSABILITY_ROT);
constexpr unsigned kOptional = kNormalLayers | kMemoLayers | kPolygonLayers;

// an id an entry point takes at all: a reference layer, or a user layer that was added
inline bool known(const Facts& f, int id) { return (id >= 0 && id < TE_LAYER_COUNT) || (id >= TE_LAYER_COUNT && (f.user_added & layer_bit(id))); }
// memory from the first write
inline bool on_demand(const Facts& f, int id) { return id == TE_LAYER_ROBOT_SLOPE || (id >= TE_LAYER_COUNT && (f.user_added & layer_bit(id))); }

inline bool input_exists(const Facts& f, int id) {
  const unsigned b = layer_bit(id);
  if (!(f.has_memory & b) || ((b & kOptional) && !(b & (kPolygonLayers | f.layers_written)))) return false;
  if (id >= TE_LAYER_COUNT) return (f.user_added & f.layers_written & b) != 0;
  return id == TE_LAYER_ROBOT_SLOPE ? f.have_robot_slope : id == TE_LAYER_ELEVATION ? f.have_elev : true;
}

// max_maps: what the launch can take in one call, 0: any number
inline Verdict check(const Facts& f, int in_layer, int out_layer, int map0, int nmaps, int max_maps) {
  if (!f.have_geo) return {TE_ERR_NOT_READY, kNoGeometry, -1, false};
  if (!known(f, out_layer)) return {TE_ERR_INVALID_ARG, kBadOutput, out_layer, false};
  // (map0 + nmaps may not be representable; batch - nmaps is: nmaps > 0 here)
  if (map0 < 0 || nmaps <= 0 || map0 > f.batch - nmaps) return {TE_ERR_INVALID_ARG, kBadMaps, -1, false};
  if (max_maps > 0 && nmaps > max_maps) return {TE_ERR_INVALID_ARG, kTooManyMaps, -1, false};
  if (!known(f, in_layer)) return {TE_ERR_INVALID_ARG, kBadInput, in_layer, false};
  if (!input_exists(f, in_layer)) return {TE_ERR_NOT_READY, kInputAbsent, in_layer, false};
  if (!on_demand(f, out_layer) && !(f.has_memory & layer_bit(out_layer))) return {TE_ERR_INVALID_ARG, kOutputNoMemory, out_layer, false};
  return {TE_OK, kAccepted, -1, in_layer == out_layer};
}

// The region form: check()'s rules for the one map, then two of its own -- a region call reads the neighbours of the rectangle
// as they were before the filter, so it never runs in place, and the rectangle lies inside the map (f.rows x f.cols).
inline Verdict check_region(const Facts& f, int in_layer, int out_layer, int map, int row0, int col0, int h, int w) {
  Verdict v = check(f, in_layer, out_layer, map, 1, 0);
  if (v.rule == kBadMaps) v.rule = kBadMap;
  if (v.code != TE_OK) return v;
  if (in_layer == out_layer) return {TE_ERR_INVALID_ARG, kRegionInPlace, in_layer, false};
  if (!region::valid_rect(f.rows, f.cols, row0, col0, h, w)) return {TE_ERR_INVALID_ARG, kBadRect, -1, false};
  return v;
}

// Operands only: one layer read, judged by input_exists
inline Verdict check_operand(const Facts& f, int id) {
  if (!known(f, id)) return {TE_ERR_INVALID_ARG, kBadInput, id, false};
  if (!input_exists(f, id)) return {TE_ERR_NOT_READY, kInputAbsent, id, false};
  return {TE_OK, kAccepted, -1, false};
}
// ... of a call that rewrites that layer in place, cell by cell, on maps of the batch or on a rectangle of one map
inline Verdict check_update(const Facts& f, int layer, int map0, int nmaps) {
  if (!f.have_geo) return {TE_ERR_NOT_READY, kNoGeometry, -1, false};
  if (map0 < 0 || nmaps <= 0 || map0 > f.batch - nmaps) return {TE_ERR_INVALID_ARG, kBadMaps, -1, false};
  return check_operand(f, layer);
}
inline Verdict check_update_region(const Facts& f, int layer, int map, int row0, int col0, int h, int w) {
  Verdict v = check_update(f, layer, map, 1);
  if (v.rule == kBadMaps) v.rule = kBadMap;
  if (v.code != TE_OK) return v;
  if (!region::valid_rect(f.rows, f.cols, row0, col0, h, w)) return {TE_ERR_INVALID_ARG, kBadRect, -1, false};
  return v;
}

// The operands of an expression (ids its compiler took from the names it knows): input_exists WITHOUT the have_elev rule --
// an expression reads the elevation as soon as it has memory, uploaded or not.  The entry points have always differed in
// this; the difference is stated here, not judged.
inline Verdict check_expression_operand(const Facts& f, int id) {
  Facts g = f;
  g.have_elev = true;
  if (!input_exists(g, id)) return {TE_ERR_NOT_READY, kOperandAbsent, id, false};
  return {TE_OK, kAccepted, -1, false};
}
// The layer an expression writes: one the context knows that has memory or gets it from this write.  It may be an operand too.
inline Verdict check_expression_output(const Facts& f, int out_layer) {
  if (!known(f, out_layer)) return {TE_ERR_INVALID_ARG, kBadOutput, out_layer, false};
  if (!on_demand(f, out_layer) && !(f.has_memory & layer_bit(out_layer))) return {TE_ERR_INVALID_ARG, kOutputNoMemory, out_layer, false};
  return {TE_OK, kAccepted, -1, false};
}

}  // namespace layer_call
}  // namespace te
