// CPU harness of te_layer_call.h, the call contract of the layer filters (tests/test_layer_call.py).  Every verdict of
// te::layer_call::check is compared with the rules restated here as a table of the layers -- written from the list in the
// header's comment, without its helpers:
//   layers   every (in, out) in [-1, TE_LAYER_COUNT]^2 under every combination of the facts that matter
//   maps     every map range of batch 2 and 3, map0 = INT_MAX, the caps 0, 2 and 65535, before and behind a bad id
//   pinned   the (code, case) pairs the three test_refusals of the GPU suite assert
//   forms    the other forms (check_region, check_operand, check_update(_region), check_expression_operand / _output) over
//            every layer id, user ids added and never added among them, the same facts, and the map and rectangle edges
#include <limits.h>
#include <stdio.h>

#include <initializer_list>

#include "te_layer_call.h"

using te::layer_call::Facts;
using te::layer_call::Verdict;

namespace {

enum Memory { kSlab, kPolygon, kOwn };                             // where a layer's memory comes from
enum Holds { kAlways, kUploaded, kWhenWritten, kWithMemory, kPresent };  // when it holds values a filter may read
struct Row {
  int id;
  Memory memory;
  Holds holds;
};
const Row kLayers[] = {
    {TE_LAYER_ELEVATION, kSlab, kUploaded},
    {TE_LAYER_SLOPE, kSlab, kAlways},
    {TE_LAYER_STEP, kSlab, kAlways},
    {TE_LAYER_ROUGHNESS, kSlab, kAlways},
    {TE_LAYER_TRAVERSABILITY, kSlab, kAlways},
    {TE_LAYER_FOOTPRINT, kSlab, kAlways},
    {TE_LAYER_NORMAL_X, kSlab, kWhenWritten},
    {TE_LAYER_NORMAL_Y, kSlab, kWhenWritten},
    {TE_LAYER_NORMAL_Z, kSlab, kWhenWritten},
    {TE_LAYER_SLOPE_FOOTPRINT, kSlab, kWhenWritten},
    {TE_LAYER_STEP_FOOTPRINT, kSlab, kWhenWritten},
    {TE_LAYER_ROUGHNESS_FOOTPRINT, kSlab, kWhenWritten},
    {TE_LAYER_TRAVERSABILITY_X, kPolygon, kWithMemory},
    {TE_LAYER_TRAVERSABILITY_ROT, kPolygon, kWithMemory},
    {TE_LAYER_ROBOT_SLOPE, kOwn, kPresent},
};
static_assert(sizeof(kLayers) / sizeof(kLayers[0]) == TE_LAYER_COUNT, "one row per layer");

// the state of a context, as the table reads it
struct World {
  bool geo, elev, polygon_memory, robot_memory, robot_present;
  unsigned written;
  int batch;
  // user layers (ids TE_LAYER_COUNT .. 30): which were added, which of them have memory; they hold values once written
  unsigned user_added, user_memory;
};
constexpr int kRows = 16, kCols = 9;  // the map of every world

const Row* row(int id) {
  for (const Row& r : kLayers)
    if (r.id == id) return &r;
  return nullptr;
}
bool memory(const World& w, const Row& r) { return r.memory == kSlab ? w.geo : r.memory == kPolygon ? w.polygon_memory : w.robot_memory; }
bool holds(const World& w, const Row& r) {
  switch (r.holds) {
    case kAlways: return true;
    case kUploaded: return w.elev;
    case kWhenWritten: return ((w.written >> r.id) & 1u) != 0;
    case kWithMemory: return true;
    case kPresent: return w.robot_present;
  }
  return false;
}

struct Want {
  int code, rule, id;
  bool in_place;
};
Want expected(const World& w, int in, int out, int map0, int nmaps, int max_maps) {
  if (!w.geo) return {TE_ERR_NOT_READY, 1, -1, false};
  if (!row(out)) return {TE_ERR_INVALID_ARG, 2, out, false};
  if (map0 < 0 || nmaps <= 0 || (long long)map0 + nmaps > w.batch) return {TE_ERR_INVALID_ARG, 3, -1, false};
  if (max_maps != 0 && nmaps > max_maps) return {TE_ERR_INVALID_ARG, 4, -1, false};
  if (!row(in)) return {TE_ERR_INVALID_ARG, 5, in, false};
  if (!memory(w, *row(in)) || !holds(w, *row(in))) return {TE_ERR_NOT_READY, 6, in, false};
  if (out != TE_LAYER_ROBOT_SLOPE && !memory(w, *row(out))) return {TE_ERR_INVALID_ARG, 7, out, false};
  return {TE_OK, 0, -1, in == out};
}

Facts facts(const World& w) {
  Facts f;
  f.have_geo = w.geo;
  f.batch = w.batch;
  for (const Row& r : kLayers)
    if (memory(w, r)) f.has_memory |= 1u << r.id;
  f.layers_written = w.written;
  f.have_robot_slope = w.robot_present;
  f.have_elev = w.elev;
  f.rows = kRows, f.cols = kCols;
  f.user_added = w.user_added;
  f.has_memory |= w.user_memory & w.user_added;  // (the memory of a layer goes with its name)
  return f;
}

long long n_cases = 0, n_failed = 0;

void compare(const World& w, int in, int out, int map0, int nmaps, int max_maps) {
  const Want e = expected(w, in, out, map0, nmaps, max_maps);
  const Verdict v = te::layer_call::check(facts(w), in, out, map0, nmaps, max_maps);
  ++n_cases;
  if (v.code == e.code && (int)v.rule == e.rule && v.id == e.id && v.in_place == e.in_place) return;
  if (++n_failed <= 10)
    printf("FAILED geo=%d elev=%d poly=%d rs=%d/%d written=0x%x batch=%d: (%d -> %d, maps %d+%d, cap %d) gives code %d rule %d id %d in_place %d, want %d %d %d %d\n",
           (int)w.geo, (int)w.elev, (int)w.polygon_memory, (int)w.robot_memory, (int)w.robot_present, w.written, w.batch, in, out, map0, nmaps, max_maps, v.code,
           (int)v.rule, v.id, (int)v.in_place, e.code, e.rule, e.id, (int)e.in_place);
}

// the bits of `written` that matter: one per optional layer (the polygon layers' do not, and are swept to show it); the
// others are set in every second world
const int kSwept[] = {TE_LAYER_NORMAL_X,           TE_LAYER_NORMAL_Y,         TE_LAYER_NORMAL_Z,          TE_LAYER_SLOPE_FOOTPRINT, TE_LAYER_STEP_FOOTPRINT,
                      TE_LAYER_ROUGHNESS_FOOTPRINT, TE_LAYER_TRAVERSABILITY_X, TE_LAYER_TRAVERSABILITY_ROT};

void layers() {
  for (int k = 0; k < (1 << 5); ++k) {
    World w;
    w.geo = k & 1, w.elev = k & 2, w.polygon_memory = k & 4, w.robot_memory = k & 8, w.robot_present = k & 16;
    w.batch = 2;
    w.user_added = w.user_memory = 0;
    for (unsigned s = 0; s < (1u << 8); ++s) {
      w.written = (s & 1u) ? 0x7fffu : 0u;  // (every other bit with the first swept one: they decide nothing)
      for (int b = 0; b < 8; ++b) w.written = (s >> b) & 1u ? w.written | 1u << kSwept[b] : w.written & ~(1u << kSwept[b]);
      for (int in = -1; in <= TE_LAYER_COUNT; ++in)
        for (int out = -1; out <= TE_LAYER_COUNT; ++out) compare(w, in, out, 0, 2, 0);
    }
  }
}

void maps() {
  const int map0s[] = {-1, 0, 1, 2, 3, INT_MAX}, nmapss[] = {-1, 0, 1, 2, 3, 4, INT_MAX}, caps[] = {0, 2, 65535};
  const int ids[][2] = {{TE_LAYER_ELEVATION, TE_LAYER_ROUGHNESS}, {TE_LAYER_ELEVATION, TE_LAYER_ELEVATION}, {TE_LAYER_ELEVATION, -1},
                        {TE_LAYER_COUNT, TE_LAYER_ROUGHNESS},     {TE_LAYER_NORMAL_X, TE_LAYER_ROUGHNESS},  {TE_LAYER_ELEVATION, TE_LAYER_TRAVERSABILITY_X}};
  World w = {true, true, false, false, false, 0u, 0};
  for (int batch : {2, 3})
    for (int map0 : map0s)
      for (int nmaps : nmapss)
        for (int cap : caps)
          for (const auto& id : ids) {
            w.batch = batch;
            compare(w, id[0], id[1], map0, nmaps, cap);
          }
  // the cap of the grid's z extent, at a batch that reaches it
  w.batch = 70000;
  for (int nmaps : {65535, 65536, 70000})
    for (int cap : caps)
      for (int map0 : {0, 1, 4465, 70000 - 65535}) compare(w, TE_LAYER_ELEVATION, TE_LAYER_ROUGHNESS, map0, nmaps, cap);
}

// tests/test_gpu_{median_fill,radius_filter,window_expression}.py, test_refusals: a context of 16 x 9 x 2
void pinned() {
  using namespace te::layer_call;
  struct Pin {
    bool geo, elev;
    int in, out, map0, nmaps, code;
    Rule rule;
  };
  const Pin pins[] = {
      {false, false, 0, 0, 0, 1, TE_ERR_NOT_READY, kNoGeometry},
      {true, false, TE_LAYER_ELEVATION, 3, 0, 2, TE_ERR_NOT_READY, kInputAbsent},
      {true, false, TE_LAYER_NORMAL_X, 3, 0, 2, TE_ERR_NOT_READY, kInputAbsent},
      {true, false, TE_LAYER_ROBOT_SLOPE, 3, 0, 2, TE_ERR_NOT_READY, kInputAbsent},
      {true, false, TE_LAYER_TRAVERSABILITY_X, 3, 0, 2, TE_ERR_NOT_READY, kInputAbsent},
      {true, false, TE_LAYER_SLOPE_FOOTPRINT, 3, 0, 2, TE_ERR_NOT_READY, kInputAbsent},
      {true, true, -1, 3, 0, 2, TE_ERR_INVALID_ARG, kBadInput},
      {true, true, 15, 3, 0, 2, TE_ERR_INVALID_ARG, kBadInput},
      {true, true, 0, -1, 0, 2, TE_ERR_INVALID_ARG, kBadOutput},
      {true, true, 0, 15, 0, 2, TE_ERR_INVALID_ARG, kBadOutput},
      {true, true, 0, 12, 0, 2, TE_ERR_INVALID_ARG, kOutputNoMemory},
      {true, true, 0, 0, -1, 1, TE_ERR_INVALID_ARG, kBadMaps},
      {true, true, 0, 0, 0, 0, TE_ERR_INVALID_ARG, kBadMaps},
      {true, true, 0, 0, 0, 3, TE_ERR_INVALID_ARG, kBadMaps},
      {true, true, 0, 0, 2, 1, TE_ERR_INVALID_ARG, kBadMaps},
      {true, true, 0, 0, 1, 2, TE_ERR_INVALID_ARG, kBadMaps},
      {true, true, 0, 0, 0, 2, TE_OK, kAccepted},
  };
  for (const Pin& p : pins)
    for (int cap : {0, 65535}) {
      Facts f;
      f.have_geo = p.geo;
      f.batch = 2;
      f.has_memory = p.geo ? 0xfffu : 0u;  // the slab's twelve layers
      f.have_elev = p.elev;
      const Verdict v = check(f, p.in, p.out, p.map0, p.nmaps, cap);
      ++n_cases;
      if (v.code == p.code && v.rule == p.rule && v.in_place == (p.code == TE_OK && p.in == p.out)) continue;
      if (++n_failed <= 10) printf("FAILED pinned (%d -> %d, maps %d+%d): code %d rule %d, want %d %d\n", p.in, p.out, p.map0, p.nmaps, v.code, (int)v.rule, p.code, (int)p.rule);
    }
}

// ---- the other forms.  The table with the user layers beside it: a user id is a layer once added, has memory of its own
// (kOwn) and holds values once written.
bool is_layer(const World& w, int id) { return row(id) || (id >= TE_LAYER_COUNT && id < 31 && ((w.user_added >> id) & 1u)); }
bool has_memory(const World& w, int id) { return row(id) ? memory(w, *row(id)) : ((w.user_memory >> id) & 1u) != 0; }
bool has_values(const World& w, int id) { return row(id) ? holds(w, *row(id)) : ((w.written >> id) & 1u) != 0; }
bool own_memory(int id) { return id == TE_LAYER_ROBOT_SLOPE || id >= TE_LAYER_COUNT; }
bool in_map(int row0, int col0, int h, int w) { return row0 >= 0 && col0 >= 0 && h > 0 && w > 0 && (long long)row0 + h <= kRows && (long long)col0 + w <= kCols; }
struct RectCase {
  int row0, col0, h, w;
};

Want expected_region(const World& w, int in, int out, int map, const RectCase& r) {
  if (!w.geo) return {TE_ERR_NOT_READY, 1, -1, false};
  if (!is_layer(w, out)) return {TE_ERR_INVALID_ARG, 2, out, false};
  if (map < 0 || map >= w.batch) return {TE_ERR_INVALID_ARG, 8, -1, false};
  if (!is_layer(w, in)) return {TE_ERR_INVALID_ARG, 5, in, false};
  if (!has_memory(w, in) || !has_values(w, in)) return {TE_ERR_NOT_READY, 6, in, false};
  if (!own_memory(out) && !has_memory(w, out)) return {TE_ERR_INVALID_ARG, 7, out, false};
  if (in == out) return {TE_ERR_INVALID_ARG, 9, in, false};
  if (!in_map(r.row0, r.col0, r.h, r.w)) return {TE_ERR_INVALID_ARG, 10, -1, false};
  return {TE_OK, 0, -1, false};
}
Want expected_operand(const World& w, int id) {
  if (!is_layer(w, id)) return {TE_ERR_INVALID_ARG, 5, id, false};
  if (!has_memory(w, id) || !has_values(w, id)) return {TE_ERR_NOT_READY, 6, id, false};
  return {TE_OK, 0, -1, false};
}
Want expected_update(const World& w, int id, int map0, int nmaps) {
  if (!w.geo) return {TE_ERR_NOT_READY, 1, -1, false};
  if (map0 < 0 || nmaps <= 0 || (long long)map0 + nmaps > w.batch) return {TE_ERR_INVALID_ARG, 3, -1, false};
  return expected_operand(w, id);
}
Want expected_update_region(const World& w, int id, int map, const RectCase& r) {
  if (!w.geo) return {TE_ERR_NOT_READY, 1, -1, false};
  if (map < 0 || map >= w.batch) return {TE_ERR_INVALID_ARG, 8, -1, false};
  const Want e = expected_operand(w, id);
  if (e.code != TE_OK) return e;
  if (!in_map(r.row0, r.col0, r.h, r.w)) return {TE_ERR_INVALID_ARG, 10, -1, false};
  return {TE_OK, 0, -1, false};
}
// an expression reads the elevation whether uploaded or not: the one difference to expected_operand (an id that is no
// layer never reaches it: the compiler knows the names)
Want expected_expression_operand(const World& w, int id) {
  const bool values = id == TE_LAYER_ELEVATION || has_values(w, id);
  if (!is_layer(w, id) || !has_memory(w, id) || !values) return {TE_ERR_NOT_READY, 11, id, false};
  return {TE_OK, 0, -1, false};
}
Want expected_expression_output(const World& w, int out) {
  if (!is_layer(w, out)) return {TE_ERR_INVALID_ARG, 2, out, false};
  if (!own_memory(out) && !has_memory(w, out)) return {TE_ERR_INVALID_ARG, 7, out, false};
  return {TE_OK, 0, -1, false};
}

void same(const char* form, const World& w, const Want& e, const Verdict& v, int a, int b, int map0, int nmaps, const RectCase& r) {
  ++n_cases;
  if (v.code == e.code && (int)v.rule == e.rule && v.id == e.id && v.in_place == e.in_place) return;
  if (++n_failed <= 10)
    printf("FAILED %s geo=%d elev=%d poly=%d rs=%d/%d written=0x%x user=0x%x/0x%x batch=%d: (%d, %d, maps %d+%d, rect (%d,%d)+(%d,%d)) gives code %d rule %d id %d in_place "
           "%d, want %d %d %d %d\n",
           form, (int)w.geo, (int)w.elev, (int)w.polygon_memory, (int)w.robot_memory, (int)w.robot_present, w.written, w.user_added, w.user_memory, w.batch, a, b, map0, nmaps,
           r.row0, r.col0, r.h, r.w, v.code, (int)v.rule, v.id, (int)v.in_place, e.code, e.rule, e.id, (int)e.in_place);
}

void forms() {
  using namespace te::layer_call;
  // every reference id, both ends, and the user ids: 15 present, 16 added with memory but never written, 17 added without
  // memory, 30 present, 18 / 20 / 29 never added (20 with a stray written bit), 31 and up no ids at all
  const int ids[] = {-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 20, 29, 30, 31, 32, 99, INT_MAX};
  const unsigned user_added = 1u << 15 | 1u << 16 | 1u << 17 | 1u << 30, user_memory = 1u << 15 | 1u << 16 | 1u << 30 | 1u << 18;
  const unsigned user_written = 1u << 15 | 1u << 30 | 1u << 20;
  const RectCase inside = {3, 2, 5, 4};
  const RectCase rects[] = {{0, 0, kRows, kCols}, {0, 0, 1, 1},        {kRows - 1, kCols - 1, 1, 1}, {-1, 0, 1, 1},       {0, -1, 1, 1},       {0, 0, 0, 1},
                            {0, 0, 1, 0},         {0, 0, -1, 1},       {0, 0, kRows + 1, 1},         {0, 0, 1, kCols + 1}, {1, 0, kRows, 1},    {0, 1, 1, kCols},
                            {kRows, 0, 1, 1},     {0, kCols, 1, 1},    {INT_MAX, 0, 1, 1},           {0, 0, INT_MAX, 1},  {1, 1, INT_MAX, 1},  {0, INT_MAX, 1, INT_MAX},
                            inside};
  const int maps1[] = {-1, 0, 1, 2, INT_MAX};
  const int ranges[][2] = {{0, 2}, {1, 1}, {0, 1}, {0, 3}, {2, 1}, {1, 2}, {0, 0}, {-1, 1}, {0, -1}, {INT_MAX, 1}, {1, INT_MAX}};
  const unsigned optional_written[] = {0u, 0x7fffu, 1u << TE_LAYER_NORMAL_Y | 1u << TE_LAYER_STEP_FOOTPRINT | 1u << TE_LAYER_TRAVERSABILITY_X,
                                       0x7fffu & ~(1u << TE_LAYER_NORMAL_Y | 1u << TE_LAYER_STEP_FOOTPRINT | 1u << TE_LAYER_TRAVERSABILITY_X)};
  for (int k = 0; k < (1 << 6); ++k) {
    World w;
    w.geo = k & 1, w.elev = k & 2, w.polygon_memory = k & 4, w.robot_memory = k & 8, w.robot_present = k & 16;
    w.batch = 2;
    w.user_added = (k & 32) ? user_added : 0u;
    w.user_memory = user_memory;
    for (unsigned written : optional_written) {
      w.written = written | user_written;
      const Facts f = facts(w);
      for (int a : ids) {
        same("operand", w, expected_operand(w, a), check_operand(f, a), a, -1, 0, 0, inside);
        if (a >= 0 && a < 31) same("expression operand", w, expected_expression_operand(w, a), check_expression_operand(f, a), a, -1, 0, 0, inside);
        same("expression output", w, expected_expression_output(w, a), check_expression_output(f, a), -1, a, 0, 0, inside);
        for (const auto& m : ranges) same("update", w, expected_update(w, a, m[0], m[1]), check_update(f, a, m[0], m[1]), a, -1, m[0], m[1], inside);
        for (int map : maps1) {
          for (const RectCase& r : {inside, rects[3], rects[8]})
            same("update region", w, expected_update_region(w, a, map, r), check_update_region(f, a, map, r.row0, r.col0, r.h, r.w), a, -1, map, 1, r);
          for (int b : ids)
            for (const RectCase& r : {inside, rects[9]})
              same("region", w, expected_region(w, a, b, map, r), check_region(f, a, b, map, r.row0, r.col0, r.h, r.w), a, b, map, 1, r);
        }
      }
    }
  }
  // the rectangle edges, on a world where every other rule passes
  World w = {true, true, false, false, false, 0u, 2, 0u, 0u};
  const Facts f = facts(w);
  for (const RectCase& r : rects) {
    same("region", w, expected_region(w, TE_LAYER_ELEVATION, TE_LAYER_ROUGHNESS, 1, r),
         check_region(f, TE_LAYER_ELEVATION, TE_LAYER_ROUGHNESS, 1, r.row0, r.col0, r.h, r.w), TE_LAYER_ELEVATION, TE_LAYER_ROUGHNESS, 1, 1, r);
    same("update region", w, expected_update_region(w, TE_LAYER_SLOPE, 0, r), check_update_region(f, TE_LAYER_SLOPE, 0, r.row0, r.col0, r.h, r.w), TE_LAYER_SLOPE, -1, 0, 1, r);
  }
}

}  // namespace

int main() {
  layers();
  maps();
  pinned();
  forms();
  printf("%lld cases, %lld failed checks\n", n_cases, n_failed);
  return n_failed ? 1 : 0;
}
