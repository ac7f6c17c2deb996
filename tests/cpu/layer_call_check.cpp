// CPU harness of te_layer_call.h, the call contract of the layer filters (tests/test_layer_call.py).  Every verdict of
// te::layer_call::check is compared with the rules restated here as a table of the layers -- written from the list in the
// header's comment, without its helpers:
//   layers   every (in, out) in [-1, TE_LAYER_COUNT]^2 under every combination of the facts that matter
//   maps     every map range of batch 2 and 3, map0 = INT_MAX, the caps 0, 2 and 65535, before and behind a bad id
//   pinned   the (code, case) pairs the three test_refusals of the GPU suite assert
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
};

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

}  // namespace

int main() {
  layers();
  maps();
  pinned();
  printf("%lld cases, %lld failed checks\n", n_cases, n_failed);
  return n_failed ? 1 : 0;
}
