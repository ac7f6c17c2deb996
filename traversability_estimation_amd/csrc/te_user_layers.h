// te_user_layers.h -- the names of a context's user layers (te_add_layer / te_remove_layer / te_layer_id / te_layer_name):
// up to TE_MAX_USER_LAYERS float layers beside the 15 of the reference, ids TE_LAYER_COUNT .. TE_LAYER_COUNT + 15, so that a
// grid_map filter chain can keep layers under its own names (elevation_filled, slope, edges, ...).  Plain C++ without HIP: the
// shim (te_ctx.h: te_ctx::user) and the CPU test (tests/cpu/user_layer_check.cpp) run the same code.  The table holds names
// only; the memory of a layer is te_ctx::LayerMem::user, which a te_set_geometry to another shape frees while the names stay.
//
// A name matches [A-Za-z_][A-Za-z0-9_]{0,62}, is none of the reference's 15 layer names and none of the names the expression
// language gives a meaning (te_expr.h: functions, reductions and the EigenLab functions it refuses by name): an operand of an
// expression must never be read as something else.  Ids are handed out lowest free first.
#pragma once
#include <string.h>

#include "te_expr.h"
#include "travgpu.h"

namespace te {
namespace user {

constexpr int kMax = TE_MAX_USER_LAYERS;
constexpr int kNameCap = 64;  // with the terminator
static_assert(TE_LAYER_COUNT + kMax <= 32, "user ids must fit the 32-bit layer masks");

inline bool is_user_id(int layer) { return layer >= TE_LAYER_COUNT && layer < TE_LAYER_COUNT + kMax; }

inline bool well_formed(const char* s) {
  if (!s) return false;
  const auto alpha = [](char c) { return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || c == '_'; };
  if (!alpha(s[0])) return false;
  size_t n = 1;
  for (; s[n]; ++n)
    if (n >= kNameCap - 1 || !(alpha(s[n]) || (s[n] >= '0' && s[n] <= '9'))) return false;
  return true;
}

// the id of a reference layer by its name, -1: none
inline int reference_id(const char* s) {
  int n = 0;
  const expr::LayerName* names = expr::layer_names(&n);
  for (int k = 0; k < n; ++k)
    if (strcmp(names[k].name, s) == 0) return names[k].id;
  return -1;
}

struct Table {
  char name[kMax][kNameCap] = {};  // "" : the id is free

  bool added(int layer) const { return is_user_id(layer) && name[layer - TE_LAYER_COUNT][0] != 0; }
  // bit `id` of every layer that was added
  unsigned mask() const {
    unsigned m = 0;
    for (int k = 0; k < kMax; ++k)
      if (name[k][0]) m |= 1u << (TE_LAYER_COUNT + k);
    return m;
  }
  // reference names too; -1: no such layer
  int find(const char* s) const {
    if (!s || !s[0]) return -1;
    const int ref = reference_id(s);
    if (ref >= 0) return ref;
    for (int k = 0; k < kMax; ++k)
      if (strcmp(name[k], s) == 0) return TE_LAYER_COUNT + k;
    return -1;
  }
  // TE_OK with *layer (an existing user name: its id), TE_ERR_BAD_PARAM (the name; *why says which rule), TE_ERR_UNSUPPORTED
  // (every id is taken)
  int add(const char* s, int* layer, const char** why) {
    *why = "";
    if (!well_formed(s)) {
      *why = "a layer name matches [A-Za-z_][A-Za-z0-9_]{0,62}";
      return TE_ERR_BAD_PARAM;
    }
    if (reference_id(s) >= 0) {
      *why = "the name is one of the reference's layers";
      return TE_ERR_BAD_PARAM;
    }
    if (expr::Compiler::is_function_name(s, strlen(s))) {
      *why = "the name is a function or reduction of the expression language";
      return TE_ERR_BAD_PARAM;
    }
    int free_k = -1;
    for (int k = 0; k < kMax; ++k) {
      if (strcmp(name[k], s) == 0) {
        *layer = TE_LAYER_COUNT + k;
        return TE_OK;
      }
      if (free_k < 0 && !name[k][0]) free_k = k;
    }
    if (free_k < 0) {
      *why = "all 16 user layers are in use";
      return TE_ERR_UNSUPPORTED;
    }
    strcpy(name[free_k], s);
    *layer = TE_LAYER_COUNT + free_k;
    return TE_OK;
  }
  // TE_ERR_INVALID_ARG: a reference layer, an id out of range, or one that was never added
  int remove(int layer) {
    if (!added(layer)) return TE_ERR_INVALID_ARG;
    name[layer - TE_LAYER_COUNT][0] = 0;
    return TE_OK;
  }
  // the names as operands of an expression (te_expr.h: Compiler::compile); returns how many
  int operands(expr::LayerName* out) const {
    int n = 0;
    for (int k = 0; k < kMax; ++k)
      if (name[k][0]) out[n++] = expr::LayerName{name[k], TE_LAYER_COUNT + k};
    return n;
  }
};

}  // namespace user
}  // namespace te
