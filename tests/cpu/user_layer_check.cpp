// user_layer_check.cpp -- the plain C++ behind the user layers, run on the CPU (tests/test_user_layers_plan.py):
//   names   te_user_layers.h: the name rules, lowest free id first, the 17th refusal, add / remove / add reuse, find
//   calls   te_layer_call.h: the call contract with ids 15 .. 30 present, absent and never added, for every class of call
//           (max_maps 0 and 65535, in place and not)
//   state   te_ctx_state.h: user_layer_written / user_layer_present change no cached result of the chain
// Prints one line per check group and "FAIL ..." lines; exit status 1 if any check failed.
#include <stdio.h>
#include <string.h>

#include <string>

#include "te_layer_call.h"
#include "te_user_layers.h"

using namespace te;

static int g_fail = 0;
#define CHECK(cond, ...)          \
  do {                            \
    if (!(cond)) {                \
      ++g_fail;                   \
      printf("FAIL %s:%d ", __FILE__, __LINE__); \
      printf(__VA_ARGS__);        \
      printf("\n");               \
    }                             \
  } while (0)

static int names() {
  user::Table t;
  const char* why = "";
  int id = -1;
  // the rules
  const char* bad[] = {"", "1abc", "a-b", "a b", "a.b", "elevation", "traversability_slope", "robot_slope", "sqrt", "cwiseMin", "meanOfFinites",
                       "min", "transpose", "sum", "acos"};
  for (const char* s : bad) CHECK(t.add(s, &id, &why) == TE_ERR_BAD_PARAM && why[0], "'%s' accepted", s);
  CHECK(t.add(nullptr, &id, &why) == TE_ERR_BAD_PARAM, "NULL accepted");
  const std::string long_ok(63, 'a'), too_long(64, 'a');
  CHECK(t.add(too_long.c_str(), &id, &why) == TE_ERR_BAD_PARAM, "64 characters accepted");
  CHECK(t.mask() == 0, "a refused name left a layer");
  CHECK(t.add(long_ok.c_str(), &id, &why) == TE_OK && id == TE_LAYER_COUNT, "63 characters: id %d", id);
  CHECK(t.remove(id) == TE_OK && t.mask() == 0, "remove");
  // lowest free first, an existing name returns its id
  const char* good[] = {"elevation_filled", "_x", "Slope2", "edges"};
  for (int k = 0; k < 4; ++k) CHECK(t.add(good[k], &id, &why) == TE_OK && id == TE_LAYER_COUNT + k, "%s: id %d", good[k], id);
  CHECK(t.add("_x", &id, &why) == TE_OK && id == TE_LAYER_COUNT + 1, "existing name: id %d", id);
  CHECK(t.find("Slope2") == TE_LAYER_COUNT + 2 && t.find("slope2") == -1 && t.find("elevation") == TE_LAYER_ELEVATION && t.find("robot_slope") == TE_LAYER_ROBOT_SLOPE,
        "find");
  // remove: reference layers and ids never added are refused; the id is reused, and so is the name
  CHECK(t.remove(TE_LAYER_ELEVATION) == TE_ERR_INVALID_ARG && t.remove(-1) == TE_ERR_INVALID_ARG && t.remove(TE_LAYER_COUNT + 9) == TE_ERR_INVALID_ARG &&
            t.remove(TE_LAYER_COUNT + user::kMax) == TE_ERR_INVALID_ARG,
        "remove of what is no user layer");
  CHECK(t.remove(TE_LAYER_COUNT + 1) == TE_OK && t.find("_x") == -1 && !t.added(TE_LAYER_COUNT + 1), "remove _x");
  CHECK(t.add("other", &id, &why) == TE_OK && id == TE_LAYER_COUNT + 1, "reuse: id %d", id);
  CHECK(t.add("_x", &id, &why) == TE_OK && id == TE_LAYER_COUNT + 4, "_x again: id %d", id);
  // the 17th
  char name[16];
  for (int k = 5; k < user::kMax; ++k) {
    snprintf(name, sizeof(name), "l%d", k);
    CHECK(t.add(name, &id, &why) == TE_OK && id == TE_LAYER_COUNT + k, "%s: id %d", name, id);
  }
  CHECK(t.mask() == 0x7fff8000u, "mask 0x%x", t.mask());
  CHECK(t.add("one_too_many", &id, &why) == TE_ERR_UNSUPPORTED, "the 17th layer was not refused");
  CHECK(t.add("l7", &id, &why) == TE_OK && id == TE_LAYER_COUNT + 7, "an existing name with the table full");
  expr::LayerName ops[user::kMax];
  CHECK(t.operands(ops) == user::kMax && ops[3].id == TE_LAYER_COUNT + 3 && strcmp(ops[3].name, "edges") == 0, "operands");
  printf("names: done\n");
  return 0;
}

// the rules restated for one call, independent of te_layer_call.h's code
static layer_call::Verdict expected(const layer_call::Facts& f, int in, int out, int map0, int nmaps, int max_maps) {
  using namespace layer_call;
  const auto is_layer = [&](int id) { return (id >= 0 && id < TE_LAYER_COUNT) || (id >= TE_LAYER_COUNT && id < 32 && (f.user_added >> id & 1)); };
  if (!f.have_geo) return {TE_ERR_NOT_READY, kNoGeometry, -1, false};
  if (!is_layer(out)) return {TE_ERR_INVALID_ARG, kBadOutput, out, false};
  if (map0 < 0 || nmaps <= 0 || map0 > f.batch - nmaps) return {TE_ERR_INVALID_ARG, kBadMaps, -1, false};
  if (max_maps > 0 && nmaps > max_maps) return {TE_ERR_INVALID_ARG, kTooManyMaps, -1, false};
  if (!is_layer(in)) return {TE_ERR_INVALID_ARG, kBadInput, in, false};
  bool exists;
  if (in >= TE_LAYER_COUNT)
    exists = (f.has_memory >> in & 1) && (f.layers_written >> in & 1);
  else
    exists = input_exists(f, in);  // (the reference layers: the rule tests/cpu/layer_call_check.cpp holds)
  if (!exists) return {TE_ERR_NOT_READY, kInputAbsent, in, false};
  const bool gets_memory = out == TE_LAYER_ROBOT_SLOPE || out >= TE_LAYER_COUNT;
  if (!gets_memory && !(f.has_memory >> out & 1)) return {TE_ERR_INVALID_ARG, kOutputNoMemory, out, false};
  return {TE_OK, kAccepted, -1, in == out};
}

static int calls() {
  using namespace layer_call;
  long n = 0;
  // user layers 15 (present), 16 (added, memory, declared absent), 17 (added, no memory), 30 (present); 18 .. 29 never added
  Facts f;
  f.have_geo = true;
  f.batch = 2;
  f.have_elev = true;
  f.has_memory = 0xfff | 1u << 15 | 1u << 16 | 1u << 30;  // the slab's layers; no polygon layers, no robot_slope
  f.layers_written = 1u << 15 | 1u << 30 | 1u << 20;      // (bit 20: a refused call touched an id that was never added)
  f.user_added = 1u << 15 | 1u << 16 | 1u << 17 | 1u << 30;
  const int ids[] = {-1, 0, 4, 6, 12, 14, 15, 16, 17, 18, 20, 29, 30, 31, 32, 99};
  const int maps[][2] = {{0, 2}, {1, 1}, {0, 3}, {2, 1}, {0, 0}, {-1, 1}};
  for (int geo = 0; geo < 2; ++geo)
    for (int max_maps : {0, 1, 65535})
      for (int in : ids)
        for (int out : ids)
          for (const auto& m : maps) {
            Facts g = f;
            g.have_geo = geo != 0;
            const Verdict got = check(g, in, out, m[0], m[1], max_maps), want = expected(g, in, out, m[0], m[1], max_maps);
            ++n;
            CHECK(got.code == want.code && got.rule == want.rule && got.id == want.id && got.in_place == want.in_place,
                  "geo=%d in=%d out=%d maps=%d+%d max=%d: got (%d, rule %d, id %d, in place %d), want (%d, rule %d, id %d, in place %d)", geo, in, out, m[0], m[1],
                  max_maps, got.code, (int)got.rule, got.id, (int)got.in_place, want.code, (int)want.rule, want.id, (int)want.in_place);
          }
  // spot checks in words
  CHECK(check(f, 15, 17, 0, 2, 0).code == TE_OK, "a present user layer into one without memory");
  CHECK(check(f, 16, 15, 0, 2, 0).code == TE_ERR_NOT_READY && check(f, 17, 15, 0, 2, 0).code == TE_ERR_NOT_READY, "an absent user layer as input");
  CHECK(check(f, 20, 15, 0, 2, 0).rule == kBadInput && check(f, 15, 20, 0, 2, 0).rule == kBadOutput, "an id never added is a bad id");
  CHECK(check(f, 30, 30, 0, 2, 0).in_place, "in place on a user layer");
  // without user layers nothing changes for the ids above the reference's
  Facts none = f;
  none.user_added = 0;
  for (int id = TE_LAYER_COUNT; id < 34; ++id)
    CHECK(check(none, id, 0, 0, 1, 0).rule == kBadInput && check(none, 0, id, 0, 1, 0).rule == kBadOutput, "id %d without user layers", id);
  printf("calls: %ld checked\n", n);
  return 0;
}

static int state() {
  CtxState s;
  // a complete chain + footprint result over a counted elevation
  s.elevation_replaced();
  s.elevation_counted(12, 3, 0.07);
  s.chain_launching(true, TE_RUN_FOOTPRINT | TE_RUN_FOOTPRINT_MEMO);
  s.chain_launched(true, TE_RUN_FOOTPRINT | TE_RUN_FOOTPRINT_MEMO);
  s.footprint_launched(true);
  const CtxState before = s;
  for (int layer = TE_LAYER_COUNT; layer < TE_LAYER_COUNT + user::kMax; ++layer) {
    CtxState t = before;
    // what an upload does (ensure_input_layer, then the write) and what a filter's note does
    t.layer_touched(layer);
    t.layer_written(layer, CtxState::kUploaded);
    CHECK(t.layers_written() == (before.layers_written() | layer_bit(layer)), "layer %d not present after a write", layer);
    CtxState u = before;
    u.user_layer_written(layer);
    CHECK(u == t, "layer %d: layer_written and user_layer_written differ", layer);
    CHECK(t.chain_done() && t.footprint_done() && t.mask_done() && !t.trav_external() && !t.trav_ptr_out() && t.invalid_cells() == 12 && t.invalid_runs() == 3 &&
              t.face_crit() == 0.07 && t.have_elev() && !t.have_robot_slope(),
          "a write to user layer %d changed a cached result", layer);
    t.layer_written(layer, CtxState::kPointerOut);
    CHECK(t == u, "layer %d: pointer out", layer);
    t.user_layer_present(layer, false);
    CHECK(t == before, "layer %d: declared absent is not the state before", layer);
    t.user_layer_present(layer, true);
    CHECK(t == u, "layer %d: declared present", layer);
  }
  // the transitions are about user layers only
  CtxState r = before;
  r.user_layer_written(TE_LAYER_SLOPE);
  r.user_layer_present(TE_LAYER_TRAVERSABILITY, true);
  CHECK(r == before, "a reference id changed the state through a user-layer transition");
  // a torn prefetch leaves a user layer absent, an arrived one present
  CtxState p = before;
  p.layer_touched(TE_LAYER_COUNT + 2);
  p.prefetch_joined(layer_bit(TE_LAYER_COUNT + 2), false);
  CHECK(p == before, "a torn prefetch of a user layer");
  p.layer_touched(TE_LAYER_COUNT + 2);
  p.prefetch_joined(layer_bit(TE_LAYER_COUNT + 2), true);
  CHECK(p.layers_written() == (before.layers_written() | layer_bit(TE_LAYER_COUNT + 2)) && p.chain_done() && p.footprint_done() && p.mask_done(), "an arrived prefetch");
  printf("state: done\n");
  return 0;
}

int main(int argc, char** argv) {
  const std::string what = argc > 1 ? argv[1] : "all";
  if (what == "names" || what == "all") names();
  if (what == "calls" || what == "all") calls();
  if (what == "state" || what == "all") state();
  printf("%d failed checks\n", g_fail);
  return g_fail ? 1 : 0;
}
