// CPU harness of te_ctx_state.h, the header the shim keeps its context's validity state with (tests/test_ctx_state.py):
//   cases          named sequences of transitions, one line each: the state, the bound of the combined layer for a fresh
//                  pass and for a later one, and whether the face flags may be passed
//   compose        graph_replayed against the launches it stands for, for every combination of the TE_RUN_* bits
//   sweep N SEED   N random sequences of entry points; the invariants after every step, and how often each transition ran
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "te_ctx_state.h"

using te::CtxState;

namespace {

constexpr double kCrit = 0.07;                       // the fp_critical_step "in force"
constexpr float kW[4] = {0.25f, 1.0f, 1.0f, 1.0f};   // weights: the bound is 0.75
constexpr unsigned kAllRun = TE_RUN_KEEP_NORMALS | TE_RUN_FOOTPRINT | TE_RUN_GENERIC_KERNELS | TE_RUN_FOOTPRINT_MEMO | TE_RUN_SEQUENTIAL | TE_RUN_NORMALS_ONLY;
const double kNaN = __builtin_nan("");

double cap(const CtxState& s, bool fresh) { return s.trav_cap(kW[0], kW[1], kW[2], kW[3], fresh); }

void upload(CtxState& s, long long cells = 12, long long runs = 3, double crit = kCrit) {
  s.elevation_replaced();
  s.elevation_counted(cells, runs, crit);
}
// te_run_chain without graph replay, as run_whole_locked sequences it
void whole_direct(CtxState& s, unsigned flags) {
  if (flags & TE_RUN_NORMALS_ONLY) flags &= ~(TE_RUN_FOOTPRINT | TE_RUN_FOOTPRINT_MEMO);
  s.chain_launching(true, flags);
  s.chain_launched(true, flags);
  if (flags & TE_RUN_FOOTPRINT) s.footprint_launched((flags & TE_RUN_FOOTPRINT_MEMO) != 0);
}
void region(CtxState& s, bool want_fp) {
  const bool mask_was_done = s.mask_done();
  s.chain_launching(false, 0);
  s.chain_launched(false, 0);
  if (want_fp) s.region_footprint_refreshed(mask_was_done);
}
void outside(CtxState& s, int layer, CtxState::Written how) {
  s.layer_touched(layer);
  s.layer_written(layer, how);
}
CtxState complete() {
  CtxState s;
  upload(s);
  whole_direct(s, TE_RUN_FOOTPRINT | TE_RUN_FOOTPRINT_MEMO);
  return s;
}

void print_case(const char* name, const CtxState& s) {
  char buf[256];
  s.dump(buf, sizeof(buf));
  printf("%s %s cap_fresh=%g cap=%g ff=%d\n", name, buf, cap(s, true), cap(s, false), (int)s.face_flags_for(kCrit, kCrit));
}

int cases() {
  using Seq = std::function<void(CtxState&)>;
  const unsigned FP = TE_RUN_FOOTPRINT, MEMO = TE_RUN_FOOTPRINT_MEMO;
  const std::vector<std::pair<const char*, Seq>> all = {
      {"fresh", [](CtxState&) {}},
      {"upload", [](CtxState& s) { upload(s); }},
      {"upload_no_flags", [](CtxState& s) { upload(s, 0, 0, kNaN); }},
      {"upload_count_failed", [](CtxState& s) { upload(s); s.elevation_replaced(); s.count_unknown(); }},
      {"complete", [](CtxState& s) { s = complete(); }},
      {"layers_freed", [](CtxState& s) { s = complete(); outside(s, TE_LAYER_ROBOT_SLOPE, CtxState::kUploaded); s.elevation_pointer_out(); s.layers_freed(); }},
      {"geometry_same_shape", [](CtxState& s) { s = complete(); s.geometry_set(); }},
      {"tile_after_complete", [](CtxState& s) { s = complete(); s.elevation_tile_written(); }},
      {"tile_first", [](CtxState& s) { s.elevation_tile_written(); }},
      {"elev_pointer_out", [](CtxState& s) { s = complete(); s.layer_touched(TE_LAYER_ELEVATION); s.elevation_pointer_out(); }},
      {"elev_pointer_then_upload", [](CtxState& s) { s = complete(); s.layer_touched(TE_LAYER_ELEVATION); s.elevation_pointer_out(); upload(s); }},
      {"touch_only", [](CtxState& s) { s.layer_touched(TE_LAYER_ROBOT_SLOPE); }},
      {"upload_robot_slope", [](CtxState& s) { outside(s, TE_LAYER_ROBOT_SLOPE, CtxState::kUploaded); }},
      {"ptr_robot_slope", [](CtxState& s) { outside(s, TE_LAYER_ROBOT_SLOPE, CtxState::kPointerOut); }},
      {"ptr_robot_slope_declared", [](CtxState& s) { outside(s, TE_LAYER_ROBOT_SLOPE, CtxState::kPointerOut); s.robot_slope_present(true); }},
      {"robot_slope_declared_absent", [](CtxState& s) { outside(s, TE_LAYER_ROBOT_SLOPE, CtxState::kUploaded); s.robot_slope_present(false); }},
      {"upload_slope_after_complete", [](CtxState& s) { s = complete(); outside(s, TE_LAYER_SLOPE, CtxState::kUploaded); }},
      {"ptr_roughness_after_complete", [](CtxState& s) { s = complete(); outside(s, TE_LAYER_ROUGHNESS, CtxState::kPointerOut); }},
      {"upload_trav_after_complete", [](CtxState& s) { s = complete(); outside(s, TE_LAYER_TRAVERSABILITY, CtxState::kUploaded); }},
      {"upload_footprint_layer", [](CtxState& s) { s = complete(); outside(s, TE_LAYER_FOOTPRINT, CtxState::kUploaded); }},
      {"trav_ptr_then_fresh_run", [FP](CtxState& s) { s = complete(); outside(s, TE_LAYER_TRAVERSABILITY, CtxState::kPointerOut); whole_direct(s, FP); }},
      {"params_fp_radius", [](CtxState& s) { s = complete(); s.params_changed(false, false, false); }},
      {"params_fp_max_gap", [](CtxState& s) { s = complete(); s.params_changed(false, true, false); }},
      {"params_fp_critical_step", [](CtxState& s) { s = complete(); s.params_changed(false, true, true); }},
      {"params_filter_part", [](CtxState& s) { s = complete(); s.params_changed(true, false, false); }},
      {"params_fp_radius_without_chain", [](CtxState& s) { upload(s); s.params_changed(false, false, false); }},
      {"prefetch_elev_failed", [](CtxState& s) { s = complete(); s.prefetch_joined(te::layer_bit(TE_LAYER_ELEVATION), false); }},
      {"prefetch_elev_ok", [](CtxState& s) { s = complete(); s.prefetch_joined(te::layer_bit(TE_LAYER_ELEVATION), true); s.count_unknown(); s.elevation_counted(5, 5, kCrit); }},
      {"prefetch_elev_ok_count_failed", [](CtxState& s) { s = complete(); s.prefetch_joined(te::layer_bit(TE_LAYER_ELEVATION), true); s.count_unknown(); }},
      {"prefetch_score_ok", [](CtxState& s) { s = complete(); s.prefetch_joined(te::layer_bit(TE_LAYER_STEP), true); }},
      {"prefetch_inputs_failed", [](CtxState& s) { s = complete(); s.prefetch_joined(te::layer_bit(TE_LAYER_TRAVERSABILITY) | te::layer_bit(TE_LAYER_ROBOT_SLOPE) | te::layer_bit(TE_LAYER_SLOPE), false); }},
      {"prefetch_inputs_ok", [](CtxState& s) { s = complete(); s.prefetch_joined(te::layer_bit(TE_LAYER_TRAVERSABILITY) | te::layer_bit(TE_LAYER_ROBOT_SLOPE), true); }},
      {"opt_fp_any_reach", [](CtxState& s) { s = complete(); s.footprint_option_changed(); }},
      {"opt_filter_any_radius", [](CtxState& s) { s = complete(); s.filter_option_changed(); }},
      {"chain_launch_failed", [FP](CtxState& s) { upload(s); s.chain_launching(true, FP); }},
      {"chain_fp_before_footprint", [FP](CtxState& s) { upload(s); s.chain_launching(true, FP); s.chain_launched(true, FP); }},
      {"chain_sequential_fp_before_footprint", [FP](CtxState& s) { upload(s); s.chain_launching(true, FP | TE_RUN_SEQUENTIAL); s.chain_launched(true, FP | TE_RUN_SEQUENTIAL); }},
      {"chain_plain", [](CtxState& s) { upload(s); whole_direct(s, 0); }},
      {"chain_keep_normals", [](CtxState& s) { upload(s); whole_direct(s, TE_RUN_KEEP_NORMALS); }},
      {"chain_drops_normals_after_keep", [](CtxState& s) { upload(s); whole_direct(s, TE_RUN_KEEP_NORMALS); whole_direct(s, 0); }},
      {"chain_normals_only", [FP, MEMO](CtxState& s) { upload(s); whole_direct(s, TE_RUN_NORMALS_ONLY | FP | MEMO); }},
      {"chain_fp_no_memo", [FP](CtxState& s) { upload(s); whole_direct(s, FP); }},
      {"chain_after_external_trav", [](CtxState& s) { s = complete(); outside(s, TE_LAYER_TRAVERSABILITY, CtxState::kUploaded); whole_direct(s, 0); }},
      {"run_footprint_after_chain", [](CtxState& s) { upload(s); whole_direct(s, 0); s.footprint_launched(true); }},
      {"region_chain", [](CtxState& s) { s = complete(); region(s, false); }},
      {"region_chain_fp", [](CtxState& s) { s = complete(); region(s, true); }},
      {"region_chain_fp_after_score_upload", [](CtxState& s) { s = complete(); outside(s, TE_LAYER_SLOPE, CtxState::kUploaded); region(s, true); }},
      {"region_keeps_external_and_normals", [](CtxState& s) { upload(s); whole_direct(s, TE_RUN_KEEP_NORMALS); outside(s, TE_LAYER_TRAVERSABILITY, CtxState::kUploaded); region(s, false); }},
      {"replay_fp_memo", [FP, MEMO](CtxState& s) { upload(s); s.graph_replayed(FP | MEMO); }},
      {"replay_plain_after_failed_footprint", [FP](CtxState& s) { upload(s); s.chain_launching(true, FP); s.chain_launched(true, FP); s.graph_replayed(0); }},
      {"filter_slope", [](CtxState& s) { s = complete(); s.filter_ran(TE_FILTER_SLOPE); }},
      {"filter_normals", [](CtxState& s) { s = complete(); s.filter_ran(TE_FILTER_NORMALS); }},
      {"filter_then_chain", [](CtxState& s) { s = complete(); s.filter_ran(TE_FILTER_COMBINE); whole_direct(s, 0); }},
      {"mask_built_after_score_upload", [](CtxState& s) { s = complete(); outside(s, TE_LAYER_SLOPE, CtxState::kUploaded); s.mask_built(); }},
      {"mask_built_takes_deferred_combine", [FP](CtxState& s) { upload(s); s.chain_launching(true, FP); s.chain_launched(true, FP); s.mask_built(); }},
      {"expression", [](CtxState& s) { s = complete(); s.expression_wrote_traversability(); }},
  };
  for (const auto& c : all) {
    CtxState s;
    c.second(s);
    print_case(c.first, s);
  }
  return 0;
}

// graph_replayed == the launches it stands for, and == what run_whole_locked's replay branch used to write out by hand
int compose() {
  int n = 0, bad = 0;
  for (unsigned flags = 0; flags < 64; ++flags) {
    if (flags & ~kAllRun) continue;
    for (int start = 0; start < 3; ++start, ++n) {
      CtxState a = complete();
      if (start == 1) { outside(a, TE_LAYER_TRAVERSABILITY, CtxState::kPointerOut); whole_direct(a, TE_RUN_KEEP_NORMALS); }
      if (start == 2) { a.filter_ran(TE_FILTER_NORMALS); a.chain_launching(true, TE_RUN_FOOTPRINT); }  // (a launch failed: combine_deferred is set)
      CtxState b = a;
      const unsigned before = a.layers_written();
      a.graph_replayed(flags);
      whole_direct(b, flags);
      const unsigned f = (flags & TE_RUN_NORMALS_ONLY) ? flags & ~(TE_RUN_FOOTPRINT | TE_RUN_FOOTPRINT_MEMO) : flags;
      const bool fp = (f & TE_RUN_FOOTPRINT) != 0;
      unsigned want = (f & (TE_RUN_KEEP_NORMALS | TE_RUN_NORMALS_ONLY)) ? before | te::kNormalLayers : before & ~te::kNormalLayers;
      if (fp && (f & TE_RUN_FOOTPRINT_MEMO)) want |= te::kMemoLayers;
      const bool by_hand = !a.trav_external() && a.chain_done() && a.footprint_done() == fp && a.mask_done() == fp && !a.combine_deferred() && a.layers_written() == want;
      if (a != b || !by_hand) {
        char x[256], y[256];
        a.dump(x, sizeof(x));
        b.dump(y, sizeof(y));
        printf("MISMATCH flags 0x%x start %d\n  replay %s\n  direct %s\n", flags, start, x, y);
        ++bad;
      }
    }
  }
  printf("%d combinations, %d mismatches\n", n, bad);
  return bad ? 1 : 0;
}

enum T {
  kLayersFreed, kGeometrySet, kElevationReplaced, kElevationCounted, kCountUnknown, kTileWritten, kElevationPointerOut, kLayerTouched,
  kLayerWritten, kRobotSlopePresent, kExpression, kPrefetchJoined, kParamsChanged, kFootprintOption, kFilterOption, kChainLaunching,
  kChainLaunched, kFootprintLaunched, kRegionFootprint, kGraphReplayed, kFilterRan, kMaskBuilt, kTransitions
};
const char* const kNames[kTransitions] = {
    "layers_freed", "geometry_set", "elevation_replaced", "elevation_counted", "count_unknown", "elevation_tile_written", "elevation_pointer_out",
    "layer_touched", "layer_written", "robot_slope_present", "expression_wrote_traversability", "prefetch_joined", "params_changed",
    "footprint_option_changed", "filter_option_changed", "chain_launching", "chain_launched", "footprint_launched", "region_footprint_refreshed",
    "graph_replayed", "filter_ran", "mask_built"};

int sweep(int n_seq, unsigned seed) {
  std::mt19937 rng(seed);
  auto pick = [&rng](unsigned n) { return (unsigned)(rng() % n); };
  long long count[kTransitions] = {0};
  long long steps = 0, failed = 0;
  auto check = [&](const CtxState& s, bool cond, const char* what) {
    if (cond) return;
    char buf[256];
    s.dump(buf, sizeof(buf));
    if (++failed <= 10) printf("FAILED %s: %s\n", what, buf);
  };
  for (int q = 0; q < n_seq; ++q) {
    CtxState s;
    const int len = 1 + (int)pick(40);
    for (int k = 0; k < len; ++k, ++steps) {
      const unsigned flags = pick(64) & kAllRun;
      bool fp_or_mask = false;  // the step ended in a footprint or mask transition
      // the entry points, each with the refusals it makes before it touches the state
      switch (pick(18)) {
        case 0:
          if (pick(4) == 0) { s.layers_freed(); ++count[kLayersFreed]; check(s, s == CtxState(), "layers_freed leaves the initial state"); }
          s.geometry_set(); ++count[kGeometrySet];
          break;
        case 1: {  // whole upload of the elevation
          s.elevation_replaced(); ++count[kElevationReplaced];
          const unsigned r = pick(8);
          if (r == 0) { s.count_unknown(); ++count[kCountUnknown]; }
          else { const long long cells = r < 3 ? 0 : (long long)pick(1000); s.elevation_counted(cells, cells ? 1 + (long long)pick((unsigned)cells) : 0, r == 1 ? kNaN : kCrit); ++count[kElevationCounted]; }
          break;
        }
        case 2: s.elevation_tile_written(); ++count[kTileWritten]; break;
        case 3: s.layer_touched(TE_LAYER_ELEVATION); ++count[kLayerTouched]; s.elevation_pointer_out(); ++count[kElevationPointerOut]; break;
        case 4: case 5: {  // upload / pointer of another layer; one in eight fails behind ensure_input_layer
          const int layer = 1 + (int)pick(TE_LAYER_COUNT - 1);
          s.layer_touched(layer); ++count[kLayerTouched];
          if (pick(8)) { s.layer_written(layer, pick(2) ? CtxState::kUploaded : CtxState::kPointerOut); ++count[kLayerWritten]; }
          break;
        }
        case 6: s.robot_slope_present(pick(2) != 0); ++count[kRobotSlopePresent]; break;
        case 7: {
          const unsigned mask = pick(1u << TE_LAYER_COUNT);
          const bool ok = pick(3) != 0;
          s.prefetch_joined(mask, ok); ++count[kPrefetchJoined];
          if (ok && (mask & 1u)) {
            if (pick(6) == 0) { s.count_unknown(); ++count[kCountUnknown]; }
            else { s.elevation_counted(pick(50), pick(50), kCrit); ++count[kElevationCounted]; }
          }
          break;
        }
        case 8: {
          const bool crit = pick(4) == 0;
          s.params_changed(pick(2) != 0, crit || pick(3) == 0, crit); ++count[kParamsChanged];
          break;
        }
        case 9:
          if (pick(2)) { s.footprint_option_changed(); ++count[kFootprintOption]; }
          else { s.filter_option_changed(); ++count[kFilterOption]; }
          break;
        case 10: case 11: {  // te_run_chain: direct, replayed, or a launch that fails
          if (!s.have_elev()) break;
          const unsigned f = (flags & TE_RUN_NORMALS_ONLY) ? flags & ~(TE_RUN_FOOTPRINT | TE_RUN_FOOTPRINT_MEMO) : flags;
          const unsigned how = pick(8);
          if (how < 3 && !(f & TE_RUN_NORMALS_ONLY)) { s.graph_replayed(f); ++count[kGraphReplayed]; fp_or_mask = (f & TE_RUN_FOOTPRINT) != 0; break; }
          s.chain_launching(true, f); ++count[kChainLaunching];
          if (how == 7) break;
          s.chain_launched(true, f); ++count[kChainLaunched];
          check(s, !s.trav_external(), "a whole-map chain makes the combined layer its own");
          if ((f & TE_RUN_FOOTPRINT) && how != 6) { s.footprint_launched((f & TE_RUN_FOOTPRINT_MEMO) != 0); ++count[kFootprintLaunched]; fp_or_mask = true; }
          break;
        }
        case 12:  // te_run_footprint
          if (!s.chain_done()) break;
          s.footprint_launched(true); ++count[kFootprintLaunched]; fp_or_mask = true;
          break;
        case 13: case 14: {  // te_run_chain_region
          const bool want_fp = pick(2) != 0;
          if (!s.chain_done() || (want_fp && !s.footprint_done())) break;
          const bool mask_was_done = s.mask_done();
          s.chain_launching(false, 0); ++count[kChainLaunching];
          s.chain_launched(false, 0); ++count[kChainLaunched];
          if (want_fp && pick(8)) { s.region_footprint_refreshed(mask_was_done); ++count[kRegionFootprint]; fp_or_mask = true; }
          break;
        }
        case 15: {
          const int filter = TE_FILTER_SLOPE + (int)pick(5);
          if ((filter == TE_FILTER_STEP || filter == TE_FILTER_ROUGHNESS || filter == TE_FILTER_NORMALS) && !s.have_elev()) break;
          s.filter_ran(filter); ++count[kFilterRan];
          break;
        }
        case 16:  // te_check_footprint_paths_radius
          if (!s.chain_done() || s.mask_done()) break;
          s.mask_built(); ++count[kMaskBuilt]; fp_or_mask = true;
          break;
        case 17: s.expression_wrote_traversability(); ++count[kExpression]; break;
      }
      check(s, !s.footprint_done() || s.chain_done(), "footprint_done implies chain_done");
      check(s, !s.mask_done() || s.chain_done(), "mask_done implies chain_done");
      check(s, !s.chain_done() || s.have_elev(), "chain_done implies have_elev");
      check(s, !fp_or_mask || !s.combine_deferred(), "no footprint or mask transition leaves combine_deferred set");
      check(s, !s.trav_external() || (cap(s, true) == -1.0 && cap(s, false) == -1.0), "no bound on a layer from outside");
      check(s, !s.trav_ptr_out() || cap(s, false) == -1.0, "no bound for a later pass once the pointer is out");
      check(s, s.trav_external() || cap(s, true) == 0.75, "a fresh pass over the chain's own layer has the weights' bound");
      check(s, !s.elev_ptr_out() || !s.face_flags_for(kCrit, kCrit), "no face flags once the elevation pointer is out");
      check(s, !s.face_flags_for(kCrit, kCrit) || s.invalid_cells() >= 0, "face flags only with a counted elevation");
      check(s, (s.invalid_cells() < 0) == (s.invalid_runs() < 0), "runs are known with the cells");
      check(s, !s.face_flags_for(kNaN, kNaN) && !s.face_flags_for(kCrit, 0.08), "face flags need both critical steps to match");
      const te::HoleCounts h = s.hole_counts(4096);
      check(s, h.cells == 4096 && h.invalid == s.invalid_cells() && h.runs == s.invalid_runs(), "hole_counts hands the counts on");
    }
  }
  printf("%d sequences, %lld steps, %lld failed checks\n", n_seq, steps, failed);
  printf("transitions: ");
  for (int t = 0; t < kTransitions; ++t) printf("%s%s %lld", t ? ", " : "", kNames[t], count[t]);
  printf("\n");
  return failed ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "cases")) return cases();
  if (argc >= 2 && !strcmp(argv[1], "compose")) return compose();
  if (argc >= 4 && !strcmp(argv[1], "sweep")) return sweep(atoi(argv[2]), (unsigned)atoi(argv[3]));
  fprintf(stderr, "usage: ctx_state_check cases | compose | sweep N SEED\n");
  return 2;
}
