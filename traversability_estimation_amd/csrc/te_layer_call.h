// te_layer_call.h -- the call contract of the layer filters (te_run_median_fill, te_run_radius_filter,
// te_run_window_expression and their te_time_*_samples): which layer a call may read, which it may write, which maps of the
// batch it may name, and whether it runs in place.  Plain C++, no HIP: the CPU test (tests/cpu/layer_call_check.cpp) holds it
// to the rules restated as a table.  It states what prepare() of te_median_api.hip, te_radius_api.hip and
// te_window_expr_api.hip each check today, rule for rule and in their order; they do not call it yet.
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

namespace te {
namespace layer_call {

// what the decision rests on
struct Facts {
  bool have_geo = false;
  int batch = 0;
  unsigned has_memory = 0;      // bit TE_LAYER_* of every layer with device memory
  unsigned layers_written = 0;  // CtxState::layers_written()
  bool have_robot_slope = false, have_elev = false;  // CtxState::have_robot_slope(), have_elev()
  unsigned user_added = 0;      // bit id of every user layer that was added (user::Table::mask())
};

// the rules in the order they are tried: the first that fails is the verdict
enum Rule { kAccepted = 0, kNoGeometry, kBadOutput, kBadMaps, kTooManyMaps, kBadInput, kInputAbsent, kOutputNoMemory };

struct Verdict {
  int code;       // the status the entry point returns
  Rule rule;
  int id;         // the layer id kBadOutput, kBadInput, kInputAbsent or kOutputNoMemory refused; -1 otherwise
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

}  // namespace layer_call
}  // namespace te
