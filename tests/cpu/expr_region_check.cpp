// CPU harness of what te_run_expression_region and te_run_chain_region_expression decide without a device
// (tests/test_expr_region_state.py):
//   expr_region_check                 the built-in checks -> "N checks, F failed checks"
//     state   te_ctx_state.h: the transition expression_wrote_traversability_region, and the sequence tile -> one-call tick
//             (te_shim.hip: chain_region_locked), with and without the footprint flag, against te_run_chain_region followed by
//             te_upload_layer_tile(TE_LAYER_TRAVERSABILITY) -- from every start a caller can be in
//     texts   te_expr.h: which texts the rectangle form refuses, by the two facts the entry points read (n_red, layer_mask)
//   expr_region_check classify TEXT   -> "OK region" | "REFUSED reduction" | "REFUSED self" | "ERR class message"
#include <stdio.h>
#include <string.h>

#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "te_ctx_state.h"
#include "te_expr.h"

using te::CtxState;

namespace {

int g_checks = 0, g_failed = 0;
void check(bool ok, const std::string& what) {
  ++g_checks;
  if (!ok) {
    ++g_failed;
    printf("FAILED: %s\n", what.c_str());
  }
}

constexpr double kCrit = 0.07;
constexpr float kW[4] = {0.25f, 1.0f, 1.0f, 1.0f};

void upload(CtxState& s) {
  s.elevation_replaced();
  s.elevation_counted(12, 3, kCrit);
}
void whole(CtxState& s, unsigned flags) {
  s.chain_launching(true, flags);
  s.chain_launched(true, flags);
  if (flags & TE_RUN_FOOTPRINT) s.footprint_launched((flags & TE_RUN_FOOTPRINT_MEMO) != 0);
}
// te_upload_layer_tile of a layer other than the elevation (te_transfer.hip)
void layer_tile(CtxState& s, int layer) {
  s.layer_touched(layer);
  s.layer_written(layer, CtxState::kUploaded);
}
// te_run_chain_region (te_shim.hip: chain_region_locked without a program); false: refused, nothing changed
bool region_chain(CtxState& s, bool want_fp) {
  if (!s.chain_done() || (want_fp && !s.footprint_done())) return false;
  const bool mask_was_done = s.mask_done();
  s.chain_launching(false, 0);
  s.chain_launched(false, 0);
  if (want_fp) s.region_footprint_refreshed(mask_was_done);
  return true;
}
// te_run_chain_region_expression: the same with the expression between the chain and the footprint half
bool one_call_tick(CtxState& s, bool want_fp) {
  if (!s.chain_done() || (want_fp && !s.footprint_done())) return false;
  const bool mask_was_done = s.mask_done();
  s.chain_launching(false, 0);
  s.chain_launched(false, 0);
  s.expression_wrote_traversability_region();
  if (want_fp) s.region_footprint_refreshed(mask_was_done);
  return true;
}

std::string dump(const CtxState& s) {
  char buf[256];
  s.dump(buf, sizeof(buf));
  return buf;
}

void state_checks() {
  using Seq = std::function<void(CtxState&)>;
  const unsigned FP = TE_RUN_FOOTPRINT, MEMO = TE_RUN_FOOTPRINT_MEMO;
  const std::vector<std::pair<const char*, Seq>> starts = {
      {"fresh", [](CtxState&) {}},
      {"uploaded", [](CtxState& s) { upload(s); }},
      {"chain", [](CtxState& s) { upload(s); whole(s, 0); }},
      {"chain_keep_normals", [](CtxState& s) { upload(s); whole(s, TE_RUN_KEEP_NORMALS); }},
      {"chain_footprint", [=](CtxState& s) { upload(s); whole(s, FP | MEMO); }},
      {"chain_expression_footprint", [](CtxState& s) { upload(s); whole(s, 0); s.expression_wrote_traversability(); s.footprint_launched(true); }},
      {"score_uploaded_behind_the_mask", [=](CtxState& s) { upload(s); whole(s, FP); layer_tile(s, TE_LAYER_SLOPE); }},
      {"trav_pointer_out", [=](CtxState& s) { upload(s); whole(s, FP); s.layer_touched(TE_LAYER_TRAVERSABILITY); s.layer_written(TE_LAYER_TRAVERSABILITY, CtxState::kPointerOut); }},
      {"params_changed_footprint_only", [=](CtxState& s) { upload(s); whole(s, FP); s.params_changed(false, true, false); }},
      {"moved", [=](CtxState& s) { upload(s); whole(s, FP); s.map_moved(true); }},
  };
  for (const auto& st : starts)
    for (int want_fp = 0; want_fp < 2; ++want_fp) {
      const std::string what = std::string(st.first) + (want_fp ? " +footprint" : "");
      CtxState a, b;
      st.second(a);
      st.second(b);
      a.elevation_tile_written();  // the tile
      b.elevation_tile_written();
      const CtxState before = a;
      const bool ran_a = one_call_tick(a, want_fp != 0);
      const bool ran_b = region_chain(b, want_fp != 0);
      if (ran_b) layer_tile(b, TE_LAYER_TRAVERSABILITY);
      check(ran_a == ran_b, what + ": refused alike");
      check(ran_a || a == before, what + ": a refused call changes no fact");
      check(!ran_a || a == b, what + ": the facts of te_run_chain_region + te_upload_layer_tile(traversability)\n  got  " + dump(a) + "\n  want " + dump(b));
      if (ran_a) {
        check(a.trav_external() && a.trav_ptr_out() && a.trav_cap(kW[0], kW[1], kW[2], kW[3], false) < 0 && a.trav_cap(kW[0], kW[1], kW[2], kW[3], true) < 0,
              what + ": the footprint half plans without a bound");
        check(a.chain_done() && a.footprint_done() == (want_fp != 0) && !a.combine_deferred() && a.invalid_cells() == -1, what + ": done-flags of a region run");
        check((a.layers_written() & te::layer_bit(TE_LAYER_TRAVERSABILITY)) != 0 && (a.layers_written() & te::kNormalLayers) == (before.layers_written() & te::kNormalLayers),
              what + ": the layer counts as touched, the normals stay as they were");
      }
    }
  // the transition alone: te_upload_layer_tile(TE_LAYER_TRAVERSABILITY), and what te_run_expression leaves
  for (const auto& st : starts) {
    CtxState a, b, c;
    st.second(a);
    st.second(b);
    st.second(c);
    a.expression_wrote_traversability_region();
    layer_tile(b, TE_LAYER_TRAVERSABILITY);
    c.expression_wrote_traversability();
    check(a == b && a == c, std::string(st.first) + ": the named transition is the tile upload of the layer");
    CtxState d;
    st.second(d);
    check(a.chain_done() == d.chain_done() && a.footprint_done() == d.footprint_done() && a.mask_done() == d.mask_done() && a.have_elev() == d.have_elev(),
          std::string(st.first) + ": the done-flags stay");
  }
}

// what te_expr_api.hip: region_expression_program decides
const char* classify(const char* text, char* err, size_t n) {
  te::expr::Program p;
  const int rc = te::expr::compile(text, &p, err, n);
  if (rc == te::expr::kBadParam) return "ERR BAD_PARAM";
  if (rc == te::expr::kUnsupported) return "ERR UNSUPPORTED";
  if (rc != te::expr::kOk) return "ERR OTHER";
  err[0] = 0;
  if (p.n_red > 0) return "REFUSED reduction";
  if (te::expr::layer_mask(p) & te::layer_bit(TE_LAYER_TRAVERSABILITY)) return "REFUSED self";
  return "OK region";
}

void text_checks() {
  char err[256];
  const std::pair<const char*, const char*> texts[] = {
      {"(1.0 * traversability_slope + 1.0 * traversability_step + 1.0 * traversability_roughness) / 3.0", "OK region"},
      {"cwiseMin(cwiseMin(traversability_slope, traversability_step), traversability_roughness)", "OK region"},
      {"cwiseMax(traversability_slope - 0.1, 0.0)", "OK region"},
      {"acos(surface_normal_z)", "OK region"},
      {"traversability_footprint * 0.5", "OK region"},  // (a layer whose NAME holds the word)
      {"0.5", "OK region"},
      {"traversability_slope - meanOfFinites(traversability_slope)", "REFUSED reduction"},
      {"traversability_slope ./ maxOfFinites(elevation)", "REFUSED reduction"},
      {"sum(traversability)", "REFUSED reduction"},  // (both: the reduction is named first)
      {"0.5 * traversability + 0.5 * traversability_step", "REFUSED self"},
      {"cwiseMin(traversability, traversability_slope)", "REFUSED self"},
      {"traversability", "REFUSED self"},
      {"traversability_slope +", "ERR BAD_PARAM"},
      {"transpose(traversability_slope)", "ERR UNSUPPORTED"},
  };
  for (const auto& t : texts) check(strcmp(classify(t.first, err, sizeof(err)), t.second) == 0, std::string(t.first) + " -> " + t.second);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 1) {
    state_checks();
    text_checks();
    printf("%d checks, %d failed checks\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
  }
  if (argc == 3 && strcmp(argv[1], "classify") == 0) {
    char err[256];
    const char* c = classify(argv[2], err, sizeof(err));
    printf("%s%s%s\n", c, err[0] ? " " : "", err);
    return 0;
  }
  fprintf(stderr, "usage: expr_region_check [classify TEXT]\n");
  return 2;
}
