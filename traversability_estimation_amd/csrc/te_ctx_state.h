// te_ctx_state.h -- which of a context's cached results still describe its resident layers: thirteen facts, and every way they
// change as a named transition.  The facts decide what an entry point refuses with TE_ERR_NOT_READY, which footprint route a
// pass takes (te_fp_route.h, through trav_cap) and which march k_normals3 runs (te_hole_routing.h, through hole_counts).
// Plain host C++ without HIP, in a header of its own: the shim (te_ctx.h: te_ctx::st) calls the transitions where the event
// happens, under the context's lock, and the CPU test (tests/cpu/ctx_state_check.cpp, tests/test_ctx_state.py) runs the
// same code.  The fields are private: nothing outside this header can assign one.  DESIGN.md 3 has the table of the
// transitions.
#pragma once
#include <math.h>
#include <stdio.h>

#include "te_hole_routing.h"
#include "travgpu.h"

namespace te {

constexpr unsigned layer_bit(int layer) { return (layer >= 0 && layer < 32) ? 1u << layer : 0u; }
constexpr unsigned kScoreLayers = layer_bit(TE_LAYER_SLOPE) | layer_bit(TE_LAYER_STEP) | layer_bit(TE_LAYER_ROUGHNESS);
constexpr unsigned kNormalLayers = layer_bit(TE_LAYER_NORMAL_X) | layer_bit(TE_LAYER_NORMAL_Y) | layer_bit(TE_LAYER_NORMAL_Z);
constexpr unsigned kMemoLayers = layer_bit(TE_LAYER_SLOPE_FOOTPRINT) | layer_bit(TE_LAYER_STEP_FOOTPRINT) | layer_bit(TE_LAYER_ROUGHNESS_FOOTPRINT);

// bound of the combined layer the chain writes (scores lie in [0, 1]); < 0: none, a weight is negative
inline double weights_cap(float w_scale, float w_slope, float w_step, float w_rough) {
  if (!(w_scale >= 0.0f && w_slope >= 0.0f && w_step >= 0.0f && w_rough >= 0.0f)) return -1.0;
  return (double)w_scale * ((double)w_slope + (double)w_step + (double)w_rough);
}

struct CtxState {
  // how a layer was written from outside: by a call that has finished writing it (an upload, an image, a median fill), or
  // by handing out its device pointer (te_device_ptr), behind which the caller writes whenever it likes
  enum Written { kUploaded, kPointerOut };

  bool have_elev() const { return have_elev_; }
  bool chain_done() const { return chain_done_; }
  bool footprint_done() const { return footprint_done_; }
  bool mask_done() const { return mask_done_; }
  bool combine_deferred() const { return combine_deferred_; }
  bool trav_external() const { return trav_external_; }
  bool trav_ptr_out() const { return trav_ptr_out_; }
  bool elev_ptr_out() const { return elev_ptr_out_; }
  long long invalid_cells() const { return invalid_cells_; }
  long long invalid_runs() const { return invalid_runs_; }
  double face_crit() const { return face_crit_; }
  bool have_robot_slope() const { return have_robot_slope_; }
  unsigned layers_written() const { return layers_written_; }

  // ---- the layers' memory ----------------------------------------------------------------------------------------------
  // The layers were freed (te_set_geometry to another shape, te_destroy): nothing is known about the new ones.
  void layers_freed() { *this = CtxState(); }
  // te_set_geometry, also with the shape held: resolution or position may have changed under the results.
  void geometry_set() { drop_results(); }
  // te_move_map has shifted every layer by whole cells and holds the new position (te_move_plan.h).  results_kept: no disc
  // of the parameters has a tie cell, so what was computed at the old position stands wherever no cell left or entered a disc
  // -- the region contract, as after elevation_tile_written: the caller hands the exposed rectangles and the trailing lines
  // to te_run_chain_region.  The count and the face flags (built per 64 x 4 tile, which a shift misaligns) are unknown, and
  // the untraversable mask counts as not built until a whole pass, a path check or a polygon call rebuilds it.  Without results_kept the
  // elevation is still shifted and valid, and everything computed from it is dropped: as a whole upload.
  void map_moved(bool results_kept) {
    if (!results_kept) {
      elevation_replaced();
      return;
    }
    count_unknown();
    mask_done_ = false;
  }

  // ---- the elevation layer ---------------------------------------------------------------------------------------------
  // Every cell of one or more maps was replaced (whole uploads, an image, a median fill into the layer).  Called once the
  // write is queued and BEFORE the pass that counts: if that pass fails -- a HIP error -- nothing computed from the
  // previous elevation is served over the new one.
  void elevation_replaced() {
    have_elev_ = true;
    drop_results();
    count_unknown();
  }
  // The pass over the whole layer (k_count_invalid) has delivered: invalid cells, their runs, and the fp_critical_step its
  // face flags were built for (NaN: it built none).
  void elevation_counted(long long cells, long long runs, double crit) {
    invalid_cells_ = cells;
    invalid_runs_ = runs;
    face_crit_ = crit;
  }
  // ... or it is about to run, has failed, or does not cover what was written.  invalid_runs is reset with invalid_cells
  // (every reader looks at invalid_cells first: te_hole_routing.h).
  void count_unknown() {
    invalid_cells_ = -1;
    invalid_runs_ = -1;
    face_crit_ = nan_();
  }
  // te_upload_tile(_async).  Tiles are not counted: the count of the last whole upload says nothing about them (dense
  // march), and neither do its face flags.  The three done-flags STAY: a tile is followed by te_run_chain_region, which
  // refreshes the results around it and needs chain_done (and footprint_done) from the last whole run -- the region
  // contract.
  void elevation_tile_written() {
    have_elev_ = true;
    count_unknown();
  }
  // te_device_ptr(TE_LAYER_ELEVATION): the caller fills the layer in place.
  void elevation_pointer_out() {
    elevation_replaced();
    elev_ptr_out_ = true;
  }

  // ---- the other layers ------------------------------------------------------------------------------------------------
  // A layer is about to be written from outside (ensure_input_layer: every upload route and te_device_ptr pass there
  // before they write).  Stays set if the call then fails.
  void layer_touched(int layer) {
    if (layer < TE_LAYER_COUNT) layers_written_ |= layer_bit(layer);  // (a user layer is present once a write has happened: user_layer_written)
  }
  // A layer other than the elevation was written from outside.  A pointer hand-out does not make robot_slope present: the
  // buffer is all NaN until the caller has filled it and says so (te_set_layer_present).
  void layer_written(int layer, Written how) {
    if (layer >= TE_LAYER_COUNT) return user_layer_written(layer);
    if (layer == TE_LAYER_ROBOT_SLOPE && how == kUploaded) have_robot_slope_ = true;
    if (layer == TE_LAYER_TRAVERSABILITY) trav_external_ = trav_ptr_out_ = true;
    if (layer_bit(layer) & kScoreLayers) mask_done_ = false;  // (the mask reads them; footprint_done stays as it was)
  }
  void robot_slope_present(bool present) { have_robot_slope_ = present; }
  // A user layer (ids TE_LAYER_COUNT and above: te_user_layers.h) was written -- an upload, a filter, an expression, a copy,
  // its pointer handed out.  It is present from now on, and NO cached result of the chain changes: no pass of the chain, the
  // footprint or the mask reads a user layer.
  void user_layer_written(int layer) {
    if (layer >= TE_LAYER_COUNT) layers_written_ |= layer_bit(layer);
  }
  // te_set_layer_present on a user layer, and te_remove_layer / te_add_layer (absent: a new layer under a reused id starts so)
  void user_layer_present(int layer, bool present) {
    if (layer < TE_LAYER_COUNT) return;
    layers_written_ = present ? layers_written_ | layer_bit(layer) : layers_written_ & ~layer_bit(layer);
  }
  // te_run_expression: as an upload of the traversability layer; the expression never passes ensure_input_layer.
  void expression_wrote_traversability() {
    layer_touched(TE_LAYER_TRAVERSABILITY);
    layer_written(TE_LAYER_TRAVERSABILITY, kUploaded);
  }
  // te_run_expression_region, and the expression of te_run_chain_region_expression: as te_upload_layer_tile of the
  // traversability layer with the same values -- the layer counts as written from outside (no bound: the footprint pass
  // behind it takes the route of any reach), and the done-flags stay as they are.
  void expression_wrote_traversability_region() {
    layer_touched(TE_LAYER_TRAVERSABILITY);
    layer_written(TE_LAYER_TRAVERSABILITY, kUploaded);
  }
  // A prefetch was joined: `mask` the layers it wrote, `ok` whether all of them arrived.  An elevation in it counts as
  // replaced, arrived or torn -- a torn one is no elevation: the next chain needs a complete upload; the caller counts an
  // arrived one next (elevation_counted / count_unknown).  What an arrived layer changes for later calls it changes only
  // once it HAS arrived; the mask goes either way.
  void prefetch_joined(unsigned mask, bool ok) {
    if (mask & layer_bit(TE_LAYER_ELEVATION)) {
      elevation_replaced();
      have_elev_ = ok;
    }
    if (!ok) layers_written_ &= ~(mask & ~(layer_bit(TE_LAYER_COUNT) - 1u));  // (a torn user layer is absent again)
    if (ok) {
      layers_written_ |= mask & ~(layer_bit(TE_LAYER_COUNT) - 1u);  // (an arrived user layer is present)
      if (mask & layer_bit(TE_LAYER_ROBOT_SLOPE)) have_robot_slope_ = true;
      if (mask & layer_bit(TE_LAYER_TRAVERSABILITY)) trav_external_ = trav_ptr_out_ = true;
    }
    if (mask & kScoreLayers) mask_done_ = false;
  }

  // ---- parameters and options ------------------------------------------------------------------------------------------
  // te_set_params, from old and new: `filters` -- anything before fp_radius differs: the filter layers are stale; when only
  // the footprint part changed they stay (traversabilityFootprint(radius, offset) with a new radius on an unchanged map).
  // `mask_inputs` -- one of the three parameters the mask reads differs (fp_max_gap, fp_critical_step,
  // fp_check_roughness).  `crit_step` -- fp_critical_step differs: the face flags were built for the one held at upload.
  void params_changed(bool filters, bool mask_inputs, bool crit_step) {
    if (filters) chain_done_ = false;
    mask_done_ = mask_done_ && chain_done_ && !mask_inputs;
    footprint_done_ = false;
    if (crit_step) face_crit_ = nan_();
  }
  // TE_OPT_FP_ANY_REACH changed
  void footprint_option_changed() { footprint_done_ = false; }
  // TE_OPT_FILTER_ANY_RADIUS changed, TE_OPT_NORMALS_RANK_RULE set
  void filter_option_changed() { drop_results(); }
  // TE_OPT_NORMALS_ALGORITHM set (area <-> raster): the chain's results are the other method's, and so are normal layers a
  // chain or TE_FILTER_NORMALS kept -- they stop counting as written until the next run writes them
  void normals_algorithm_set() {
    drop_results();
    layers_written_ &= ~kNormalLayers;
  }

  // ---- launches --------------------------------------------------------------------------------------------------------
  // A chain is about to be launched over the whole map or a region, with the TE_RUN_* flags it will run with.  Returns
  // combine_deferred: a whole-map run with the footprint pass right behind leaves the combined layer to the mask kernel.
  // (Stays set if the launch, or the footprint pass, then fails: the layer is still unwritten.)
  bool chain_launching(bool whole, unsigned flags) {
    combine_deferred_ = whole && !(flags & TE_RUN_SEQUENTIAL) && (flags & TE_RUN_FOOTPRINT);
    return combine_deferred_;
  }
  // ... and was.  The layers the footprint pass reads have changed; after a whole-map run every cell of the combined layer
  // comes from the chain, and the normal layers are kept with TE_RUN_KEEP_NORMALS and dropped without, like the
  // DeletionFilter (a region run leaves both facts alone).
  void chain_launched(bool whole, unsigned flags) {
    chain_done_ = true;
    footprint_done_ = false;
    mask_done_ = false;
    if (!whole) return;
    trav_external_ = false;
    if (flags & (TE_RUN_KEEP_NORMALS | TE_RUN_NORMALS_ONLY))
      layers_written_ |= kNormalLayers;
    else
      layers_written_ &= ~kNormalLayers;
  }
  // A whole-map footprint pass was launched; `memo`: it wrote the three memo layers too.
  void footprint_launched(bool memo) {
    combine_deferred_ = false;
    footprint_done_ = true;
    mask_done_ = true;
    if (memo) layers_written_ |= kMemoLayers;
  }
  // te_run_chain_region with the footprint flag: the footprint layer was complete before the region's chain and is
  // refreshed where it could change, and likewise the mask -- `mask_was_done`, as found before that chain: not if a
  // score layer was uploaded since the mask was built.
  void region_footprint_refreshed(bool mask_was_done) {
    footprint_done_ = true;
    mask_done_ = mask_was_done;
  }
  // A captured whole-map launch was replayed: what the launches it holds would have left.
  void graph_replayed(unsigned flags) {
    if (flags & TE_RUN_NORMALS_ONLY) flags &= ~(TE_RUN_FOOTPRINT | TE_RUN_FOOTPRINT_MEMO);
    chain_launching(true, flags);
    chain_launched(true, flags);
    if (flags & TE_RUN_FOOTPRINT) footprint_launched((flags & TE_RUN_FOOTPRINT_MEMO) != 0);
  }
  // te_run_filter: a single plugin's filter overwrites score layers from whatever inputs are resident (TE_FILTER_NORMALS
  // also slope and roughness, with the normals radius): the layers no longer form one chain result, so region re-filters,
  // the footprint pass and the path checks must not build on them, and the combined layer has no bound.
  void filter_ran(int filter) {
    drop_results();
    trav_external_ = true;
    if (filter == TE_FILTER_NORMALS) layers_written_ |= kNormalLayers;
  }
  // A reader of the mask outside a footprint pass -- te_check_footprint_paths_radius, the four polygon entry points -- found
  // it not done and built it on its own (and with it a deferred combined layer): ensure_mask, te_paths_api.hip.
  void mask_built() {
    combine_deferred_ = false;
    mask_done_ = true;
  }

  // ---- questions -------------------------------------------------------------------------------------------------------
  // Bound of the combined layer for a footprint pass, -1: none.  `fresh`: the pass runs right behind a whole-map chain in
  // the same entry point, which rewrote EVERY cell -- the only pass that may still assume the bound once the pointer is out.
  double trav_cap(float w_scale, float w_slope, float w_step, float w_rough, bool fresh) const {
    if (trav_external_ || (trav_ptr_out_ && !fresh)) return -1.0;
    return weights_cap(w_scale, w_slope, w_step, w_rough);
  }
  // The face flags describe the resident elevation for the critical step in force: `a`, `b` -- the caller's two copies of it
  // (footprint tables, parameters).  Unknown (NaN) compares false.
  bool face_flags_for(double a, double b) const { return !elev_ptr_out_ && face_crit_ == a && face_crit_ == b; }
  // the counts te_hole_routing.h routes with; `cells`: those of the layer, all maps
  HoleCounts hole_counts(long long cells) const { return HoleCounts{cells, invalid_cells_, invalid_runs_}; }

  bool operator==(const CtxState& o) const {
    return have_elev_ == o.have_elev_ && chain_done_ == o.chain_done_ && footprint_done_ == o.footprint_done_ && mask_done_ == o.mask_done_ &&
           combine_deferred_ == o.combine_deferred_ && trav_external_ == o.trav_external_ && trav_ptr_out_ == o.trav_ptr_out_ &&
           elev_ptr_out_ == o.elev_ptr_out_ && invalid_cells_ == o.invalid_cells_ && invalid_runs_ == o.invalid_runs_ &&
           (face_crit_ == o.face_crit_ || (face_crit_ != face_crit_ && o.face_crit_ != o.face_crit_)) &&
           have_robot_slope_ == o.have_robot_slope_ && layers_written_ == o.layers_written_;
  }
  bool operator!=(const CtxState& o) const { return !(*this == o); }
  // one line, for the harness
  int dump(char* buf, size_t n) const {
    return snprintf(buf, n, "elev=%d chain=%d fp=%d mask=%d defer=%d ext=%d tptr=%d eptr=%d cells=%lld runs=%lld crit=%g rs=%d written=0x%x",
                    (int)have_elev_, (int)chain_done_, (int)footprint_done_, (int)mask_done_, (int)combine_deferred_, (int)trav_external_,
                    (int)trav_ptr_out_, (int)elev_ptr_out_, invalid_cells_, invalid_runs_, face_crit_, (int)have_robot_slope_, layers_written_);
  }

 private:
  static double nan_() { return __builtin_nan(""); }
  void drop_results() { chain_done_ = footprint_done_ = mask_done_ = false; }

  // an elevation that covers the maps a chain reads is resident
  bool have_elev_ = false;
  // the filter layers are one chain's result over the resident elevation, for the parameters held
  bool chain_done_ = false;
  // ... and the footprint layer is complete over them
  bool footprint_done_ = false;
  // The untraversable mask (Layers::untrav) is complete for the scores and the three parameters it reads (fp_max_gap,
  // fp_critical_step, fp_check_roughness).  Set by every footprint pass and by te_check_footprint_paths_radius and the polygon
  // entry points, which build the mask on their own when it is not; cleared wherever footprint_done is cleared -- except that params_changed keeps it
  // when nothing the mask reads changed -- and by a write to a score layer (which leaves footprint_done as it was).
  bool mask_done_ = false;
  // the chain left the combined layer to the mask kernel of the footprint pass behind it, which has not run yet
  bool combine_deferred_ = false;
  // The traversability layer was written from outside (upload, device pointer, a per-plugin combine of uploaded scores):
  // its values are then not bounded by the weights, and neither the fixed-point footprint kernels nor the double kernels,
  // which pack the untraversable count into the sum, may be used (te_fp_route.h: the route of any reach).
  bool trav_external_ = false;
  // te_device_ptr handed out the traversability layer: the caller may write it at any time from then on, so only a
  // footprint pass that runs right behind a chain that rewrote EVERY cell (te_run_chain with the footprint flag) may
  // still assume the bound; te_run_footprint and region runs plan without one and take the route of any reach
  // (te_fp_route.h).  Reset with the layers.  (Set by every other outside write too: nothing tells them apart later.)
  bool trav_ptr_out_ = false;
  // te_device_ptr handed out the elevation layer: the caller may write it at any time from then on, behind any later
  // upload's pass -- the face flags are never passed again until the layers are allocated anew.
  bool elev_ptr_out_ = false;
  // invalid cells of the elevation layer as of the last whole upload (-1: unknown -- tiles, device pointer), and their runs
  // in memory order (k_count_invalid)
  long long invalid_cells_ = -1;
  long long invalid_runs_ = -1;
  // Face flags (te_face_flags.h): built by the same pass over the whole elevation layer, for the fp_critical_step held
  // then -- this value; NaN: unknown -- whatever makes invalid_cells unknown, or a te_set_params that changed
  // fp_critical_step.
  double face_crit_ = __builtin_nan("");
  // the optional input layer robot_slope holds values (checkInclination)
  bool have_robot_slope_ = false;
  // Bit TE_LAYER_* of the optional layers that hold values: surface_normal_* (chain_launched, filter_ran), the three memo
  // layers (footprint_launched) and any layer an upload or te_device_ptr touched (layer_touched).  Read by
  // te_run_expression and te_run_median_fill only; cleared with the layers.
  unsigned layers_written_ = 0;
};

}  // namespace te
