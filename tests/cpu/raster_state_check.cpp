// raster_state_check.cpp -- CtxState::normals_algorithm_set (te_ctx_state.h), the transition te_set_option runs for
// TE_OPT_NORMALS_ALGORITHM: the chain's results and the kept normals stop counting as current, and nothing else moves.
// Plain C++ over the header the shim uses; tests/test_cabi_raster.py.  Prints "N checks, F failed".
#include <cstdio>

#include "te_ctx_state.h"

using namespace te;

namespace {

int n_checks = 0, n_failed = 0;
void req(bool ok, const char* what) {
  ++n_checks;
  if (!ok) {
    ++n_failed;
    printf("FAIL %s\n", what);
  }
}

void upload(CtxState& s) {
  s.elevation_replaced();
  s.elevation_counted(12, 3, 0.07);
}
void whole(CtxState& s, unsigned flags) {
  if (flags & TE_RUN_NORMALS_ONLY) flags &= ~(TE_RUN_FOOTPRINT | TE_RUN_FOOTPRINT_MEMO);
  s.chain_launching(true, flags);
  s.chain_launched(true, flags);
  if (flags & TE_RUN_FOOTPRINT) s.footprint_launched((flags & TE_RUN_FOOTPRINT_MEMO) != 0);
}

}  // namespace

int main() {
  static_assert(TE_OPT_NORMALS_ALGORITHM == 13, "travgpu.h: the option's number is part of the ABI");
  // after a complete run that kept the normals
  {
    CtxState s;
    upload(s);
    s.layer_touched(TE_LAYER_ROBOT_SLOPE);
    s.layer_written(TE_LAYER_ROBOT_SLOPE, CtxState::kUploaded);
    whole(s, TE_RUN_KEEP_NORMALS | TE_RUN_FOOTPRINT | TE_RUN_FOOTPRINT_MEMO);
    req(s.chain_done() && s.footprint_done() && s.mask_done() && (s.layers_written() & kNormalLayers) == kNormalLayers, "a complete run that kept the normals");
    const CtxState before = s;
    s.normals_algorithm_set();
    req(!s.chain_done() && !s.footprint_done() && !s.mask_done(), "the results are dropped");
    req((s.layers_written() & kNormalLayers) == 0, "the kept normals no longer count as written");
    req((s.layers_written() & kMemoLayers) == kMemoLayers && (s.layers_written() & layer_bit(TE_LAYER_ROBOT_SLOPE)), "the other written layers stay");
    req(s.have_elev() && s.invalid_cells() == before.invalid_cells() && s.invalid_runs() == before.invalid_runs() && s.face_crit() == before.face_crit() &&
            s.have_robot_slope() == before.have_robot_slope() && s.trav_external() == before.trav_external() && s.trav_ptr_out() == before.trav_ptr_out() &&
            s.elev_ptr_out() == before.elev_ptr_out() && s.combine_deferred() == before.combine_deferred(),
        "the elevation, its counts and the outside writes stay");
    // the next run makes them current again
    whole(s, TE_RUN_KEEP_NORMALS);
    req(s.chain_done() && (s.layers_written() & kNormalLayers) == kNormalLayers, "the next chain writes them again");
  }
  // after TE_FILTER_NORMALS
  {
    CtxState s;
    upload(s);
    s.filter_ran(TE_FILTER_NORMALS);
    req((s.layers_written() & kNormalLayers) == kNormalLayers, "TE_FILTER_NORMALS leaves the normals written");
    s.normals_algorithm_set();
    req((s.layers_written() & kNormalLayers) == 0 && s.trav_external(), "... which the other method's do not count as");
  }
  // normals a caller uploaded are the other method's as little as the chain's: they go too (one mask, nothing tells them apart)
  {
    CtxState s;
    upload(s);
    s.layer_touched(TE_LAYER_NORMAL_Z);
    s.layer_written(TE_LAYER_NORMAL_Z, CtxState::kUploaded);
    s.normals_algorithm_set();
    req((s.layers_written() & kNormalLayers) == 0, "an uploaded normal layer");
  }
  // on a fresh context, and set twice: as set once
  {
    CtxState s, fresh;
    s.normals_algorithm_set();
    req(s == fresh, "a fresh context stays fresh");
    upload(s);
    whole(s, 0);
    s.normals_algorithm_set();
    CtxState once = s;
    s.normals_algorithm_set();
    req(s == once, "idempotent");
    req(s.trav_cap(0.25f, 1.0f, 1.0f, 1.0f, false) == 0.75, "the combined layer keeps its bound for the next chain");
  }
  // it drops what filter_option_changed drops, and the normals on top
  {
    CtxState a, b;
    upload(a);
    whole(a, TE_RUN_FOOTPRINT);
    b = a;
    a.filter_option_changed();
    b.normals_algorithm_set();
    req(a == b, "without kept normals: the same as setting TE_OPT_NORMALS_RANK_RULE");
  }
  printf("%d checks, %d failed\n", n_checks, n_failed);
  return n_failed ? 1 : 0;
}
