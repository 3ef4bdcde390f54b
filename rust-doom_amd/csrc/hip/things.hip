// What each player sees, touches and collects of its level's things (include/rdoom.h "things"): the device
// thing set, and rdoom_world_sense_things / rdoom_worldset_sense_things.  The thing table itself is the host walker's
// (csrc/host/wad_visitor.cpp) and world.hip's handles lend it.
//
// Arithmetic: binary32, the contract's operations in the contract's order; the build passes -ffp-contract=off and HIP's division
// and square root are correctly rounded, so an IEEE host evaluating the header's expressions gets the same bits
// (tests/things_ref.py does).
//
// Shape: one 256-thread workgroup per player, as reveal.hip has it, so the state, the yaw, the level slot and the row of offsets
// are the workgroup's.  The things are taken 256 at a time; thread t of pass k evaluates thing 256 k + t.  The candidates for sight
// of a pass -- not collected, in range, in the field of view -- are appended (world_shared.hpp's append) to the `rays` array as
// vel = (dx, dz), sight.hpp's sight_limits gives every one of them its T_r over the level's blocking lines, and each candidate
// reads its own back: visible is T_r == 1.  A pass without a candidate skips sight_limits (it divides by the ray count); the
// count it decides by is read from LDS as a scalar, so the branch is the workgroup's and every barrier is reached by every thread.
// A wave holds 64 consecutive things: its ballots are two whole words of a row, wave w of pass k owns words 8 k + 2 w and
// 8 k + 2 w + 1 of all three rows, and lanes 0 and 32 load and store them.  The counts are population counts of masked ballots,
// the nearest thing of a category is a minimum over the key (bits of d2) << 32 | index -- a non-negative binary32 orders as its
// bits, so the lowest index wins among equals -- within the wave by shuffles, carried across the passes in lane k of the wave for
// category k, and across the four waves through LDS.  No atomics anywhere, and every store is a plain vector store.
// Scalar registers are what this kernel is short of (sight_limits is inlined with the line table's four arrays): a thread keeps
// its own row and record pointers, and the touch test's uniforms are parked in LDS, so that nothing spills.
#include <hip/hip_runtime.h>

#include <cmath>
#include <memory>
#include <vector>

#include "../common.hpp"
#include "kernels.hpp"
#include "player_quat.hpp"
#include "sight.hpp"
#include "thingset.hpp"
#include "world_shared.hpp"

#pragma clang fp contract(off)

namespace {

using rdoom_dev::append;
using rdoom_dev::Appended;
using rdoom_dev::LineTable;
using rdoom_dev::live_height;
using rdoom_dev::sincos_rd;
using rdoom_dev::ThingSenseArgs;
using rdoom_dev::with_level;

constexpr uint32_t WAVE = 64, THREADS = rdoom_dev::SIGHT_THREADS, WAVES = THREADS / WAVE;
constexpr uint32_t CATEGORIES = 8;                 // RDOOM_THING_DECORATION .. RDOOM_THING_UNKNOWN
constexpr uint32_t MAX_THINGS = 1u << 20;          // of a level of a set
constexpr uint64_t NO_KEY = ~0ull;                 // above every key: d2's bits are at most +inf's

// the smallest key of the wave, in every lane
__device__ __forceinline__ uint64_t wave_min_key(uint64_t key) {
#pragma unroll
  for (uint32_t o = WAVE / 2; o; o >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)key, o), hi = __shfl_xor((uint32_t)(key >> 32), o);
    const uint64_t other = (uint64_t)hi << 32 | lo;
    key = other < key ? other : key;
  }
  // the same in every lane: read as the scalars they are
  return (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(key >> 32)) << 32 | __builtin_amdgcn_readfirstlane((uint32_t)key);
}

// player p against things [first_thing, first_thing + n_things) of the set and lines [first_line, first_line + n_lines) of the
// table.  A slot outside the set comes here with no thing and no line: no word of its rows is touched
__device__ __forceinline__ void sense_player(const ThingSenseArgs &a, const LineTable &lines, uint32_t p, uint32_t first_thing,
                                             uint32_t n_things, uint32_t first_line, uint32_t n_lines) {
  __shared__ float4 list[THREADS];  // sight_limits' blocking lines
  __shared__ float4 rays[THREADS];  // the pass's candidates: dx, dz, T_r
  __shared__ float part[THREADS];   // sight_limits' minima
  __shared__ uint32_t wave_count[WAVES];
  __shared__ uint64_t wave_best[WAVES][CATEGORIES];
  __shared__ uint32_t wave_new[WAVES][CATEGORIES];
  // what a thread reads once a pass and no scalar register is kept for through sight_limits: the touch test's and the view's
  __shared__ float parked[6];  // touch_radius, -touch_below, touch_above, cos_half_fov, pos.y, collect_mask as bits

  const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1), wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const rdoom_player_state *st = a.states + p;
  const float px = st->pos[0], pz = st->pos[2];
  float s, c;
  sincos_rd(st->yaw, s, c);
  const float fx = -s, fz = -c;  // the map's forward; its right is (c, -s)
  const float *off = a.offsets ? a.offsets + (size_t)p * a.n_objects * 3 : nullptr;
  // a thread's own word of the three rows in pass 0, and its own thing: kept per thread, so that the row's base, the three
  // pointers and the table's need no scalar register through the loop
  const size_t mine = (size_t)p * a.stride + (tid >> 5);
  uint32_t *const collected = a.collected ? a.collected + mine : nullptr;
  uint32_t *const visible_out = a.visible_out ? a.visible_out + mine : nullptr;
  uint32_t *const touched_out = a.touched_out ? a.touched_out + mine : nullptr;
  // and the record and the count a thread below 8 writes at the end (tid & 7: an address inside the player's eight for every thread)
  rdoom_thing_nearest *const nearest_out = a.nearest_out ? a.nearest_out + (size_t)p * CATEGORIES + (tid & 7u) : nullptr;
  uint32_t *const new_out = a.new_out ? a.new_out + (size_t)p * CATEGORIES + (tid & 7u) : nullptr;
  const uint32_t words = (n_things + 31u) / 32u;  // of the level: no word of a row at or beyond it is touched
  const float range2 = a.max_range * a.max_range;
  const float player_size = (__builtin_fabsf(px) + __builtin_fabsf(pz)) + a.max_range;
  const uint4 *const record = reinterpret_cast<const uint4 *>(a.things + first_thing + tid);  // two words of 16 bytes a thing

  if (tid == 0) {
    parked[0] = a.touch_radius, parked[1] = -a.touch_below, parked[2] = a.touch_above, parked[3] = a.cos_half_fov, parked[4] = st->pos[1];
    parked[5] = __uint_as_float(a.collect_mask);
  }
  __syncthreads();

  // lane k < 8 of a wave keeps category k: the wave's nearest visible thing of it so far, and what the wave collected of it
  uint64_t best = NO_KEY;
  uint32_t fresh = 0u;

  for (uint32_t base = 0; base < n_things; base += THREADS) {
    const uint32_t i = base + tid;         // i < 2^20 + 256
    const uint32_t word = i >> 5;          // lanes 0 and 32 own the wave's two words
    const bool writer = (lane & 31u) == 0 && word < words;
    const uint32_t old = writer && collected ? collected[base >> 5] : 0u;
    const uint32_t old_lo = __builtin_amdgcn_readlane(old, 0), old_hi = __builtin_amdgcn_readlane(old, 32);
    const bool examined = i < n_things && !(((lane < 32 ? old_lo : old_hi) >> (lane & 31u)) & 1u);

    float dx = 0.0f, dz = 0.0f, d2 = 0.0f;
    uint32_t category = 0;
    bool touched = false, candidate = false;
    if (examined) {
      const uint4 lo = record[2 * (size_t)base], hi = record[2 * (size_t)base + 1];  // thing i = base + tid
      const float x = __uint_as_float(lo.x), z = __uint_as_float(lo.y), height = __uint_as_float(lo.z), radius = __uint_as_float(lo.w);
      category = hi.w & 7u;  // the low half of the word is `category`, whose low byte the create call holds to 0 .. 7
      dx = x - px, dz = z - pz;
      d2 = dx * dx + dz * dz;
      const float y = live_height(height, hi.x, off, a.n_objects);
      const float dy = parked[4] - y;
      const float tr = parked[0] + radius;
      touched = d2 <= tr * tr && dy >= parked[1] && dy <= parked[2];
      const float cos_half_fov = parked[3];
      const bool in_view = cos_half_fov <= -1.0f || dx * fx + dz * fz >= cos_half_fov * __builtin_sqrtf(d2);
      candidate = d2 <= range2 && in_view;
    }

    // ---- the candidates' T_r
    const Appended at = append<WAVES>(candidate, lane, wave, wave_count, 0u);
    if (candidate) rays[at.slot] = make_float4(dx, dz, 1.0f, 0.0f);  // at.slot < at.total <= 256
    __syncthreads();
    if (at.total)  // the workgroup's: at.total is a sum of scalars read from LDS
      rdoom_dev::sight_limits(lines, off, a.n_objects, first_line, n_lines, px, pz, a.max_range, player_size, at.total, list, rays, part,
                              wave_count);
    const bool visible = candidate && rays[candidate ? at.slot : 0u].z == 1.0f;  // (the next pass's stores come behind append's barrier)

    // ---- the bits: a wave's ballots are two words of each row
    const bool collects = touched && ((__float_as_uint(parked[5]) >> category) & 1u);
    const uint64_t seen = __builtin_amdgcn_ballot_w64(visible), felt = __builtin_amdgcn_ballot_w64(touched);
    const uint64_t taken = __builtin_amdgcn_ballot_w64(collects);
    if (writer) {
      const uint32_t shift = lane & 32u;
      if (visible_out) visible_out[base >> 5] = (uint32_t)(seen >> shift);  // word (base + tid) / 32 of the row
      if (touched_out) touched_out[base >> 5] = (uint32_t)(felt >> shift);
      const uint32_t bits = (uint32_t)(taken >> shift);
      if (collected && bits) collected[base >> 5] = old | bits;
    }

    // ---- per category: what was collected, and the nearest visible thing
    const uint64_t key = visible ? (uint64_t)__float_as_uint(d2) << 32 | i : NO_KEY;
#pragma nounroll  // (unrolled, the sixteen ballots are live together and the scalar registers run out)
    for (uint32_t k = 0; k < CATEGORIES; k++) {
      const bool mine = category == k;
      if (taken) {  // the wave's, as the next branch: a ballot is the same in every lane
        const uint32_t count = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(collects && mine));
        fresh += lane == k ? count : 0u;
      }
      if (__builtin_amdgcn_ballot_w64(visible && mine)) {
        const uint64_t least = wave_min_key(mine ? key : NO_KEY);
        best = lane == k && least < best ? least : best;
      }
    }
  }

  // ---- across the four waves
  if (lane < CATEGORIES) wave_best[wave][lane] = best, wave_new[wave][lane] = fresh;
  __syncthreads();
  if (tid < CATEGORIES) {
    if (new_out) *new_out = (wave_new[0][tid] + wave_new[1][tid]) + (wave_new[2][tid] + wave_new[3][tid]);
    if (nearest_out) {
      uint64_t least = wave_best[0][tid];
#pragma unroll
      for (uint32_t w = 1; w < WAVES; w++) least = wave_best[w][tid] < least ? wave_best[w][tid] : least;
      rdoom_thing_nearest *out = nearest_out;
      if (least == NO_KEY) {
        out->index = -1, out->d2 = __builtin_inff(), out->right = 0.0f, out->forward = 0.0f;
      } else {
        const uint32_t i = (uint32_t)least;  // a key's index is below n_things
        const uint4 thing = record[2 * ((ptrdiff_t)i - (ptrdiff_t)tid)];  // record is thing tid's
        const float dx = __uint_as_float(thing.x) - px, dz = __uint_as_float(thing.y) - pz;
        out->index = (int32_t)i, out->d2 = __uint_as_float((uint32_t)(least >> 32));
        out->right = dx * c + dz * fx, out->forward = dx * fx + dz * fz;
      }
    }
  }
}

__global__ __launch_bounds__(THREADS) void sense_things_kernel(ThingSenseArgs a, LineTable lines, uint2 things, uint32_t n_lines) {
  sense_player(a, lines, blockIdx.x, things.x, things.y, 0u, n_lines);
}

// the world set's: player p is in level level_of[p] of both sets; a slot outside them has no thing and no row
__global__ __launch_bounds__(THREADS) void worldset_sense_things_kernel(ThingSenseArgs a, LineTable lines, const uint2 *__restrict__ line_levels,
                                                                        const uint2 *__restrict__ thing_levels,
                                                                        const uint32_t *__restrict__ level_of, uint32_t n_levels) {
  const uint32_t p = blockIdx.x;
  const uint32_t lv = level_of[p];
  uint32_t first_line = 0, n_lines = 0, first_thing = 0, n_things = 0;
  if (lv < n_levels)
    with_level(lv, [&](uint32_t slot) __attribute__((always_inline)) {
      first_line = line_levels[slot].x, n_lines = line_levels[slot].y;
      first_thing = thing_levels[slot].x, n_things = thing_levels[slot].y;
    });
  sense_player(a, lines, p, first_thing, n_things, first_line, n_lines);
}

bool is_finite(float v) { return std::isfinite(v); }

// the arguments of a sensing launch, checked, as the kernel takes them.  noun: "world" or "world set".  What needs no thing set is
// checked first and the handle's device before the set is read, so that a host-only handle is refused whatever the set is
rdoom_status sense_args(const rdoom::MapSource &src, const char *noun, const char *the_noun, const rdoom_thingset *things,
                        const rdoom_player_state *d_states, const uint32_t *d_levels, bool needs_levels, uint32_t n, const float *d_offsets,
                        uint32_t n_objects, const rdoom_thing_sense *params, uint32_t *d_collected, uint32_t *d_visible_out,
                        uint32_t *d_touched_out, uint32_t stride, rdoom_thing_nearest *d_nearest_out, uint32_t *d_new_out, ThingSenseArgs &a) {
  if (!things || !params) return rdoom::fail(RDOOM_BAD_ARG, "null thing set or params");
  if (n && (!d_states || (needs_levels && !d_levels))) return rdoom::fail(RDOOM_BAD_ARG, "null states or levels with n = %u", n);
  if (!d_collected && !d_visible_out && !d_touched_out && !d_nearest_out && !d_new_out)
    return rdoom::fail(RDOOM_BAD_ARG, "every output is null: nothing to sense");
  if (!(params->max_range > 0.0f) || !is_finite(params->max_range))
    return rdoom::fail(RDOOM_BAD_ARG, "max_range %g is not a finite positive number", (double)params->max_range);
  if (!is_finite(params->cos_half_fov)) return rdoom::fail(RDOOM_BAD_ARG, "cos_half_fov %g is not finite", (double)params->cos_half_fov);
  if (!(params->touch_radius >= 0.0f) || !is_finite(params->touch_radius))
    return rdoom::fail(RDOOM_BAD_ARG, "touch_radius %g is not a finite number >= 0", (double)params->touch_radius);
  if (!(params->touch_below >= 0.0f) || !(params->touch_above >= 0.0f))
    return rdoom::fail(RDOOM_BAD_ARG, "a vertical window of %g below and %g above (each >= 0)", (double)params->touch_below,
                       (double)params->touch_above);
  if (params->flags) return rdoom::fail(RDOOM_BAD_ARG, "flags %#x: none is defined", params->flags);
  if (n > 0x7FFFFFFFu) return rdoom::fail(RDOOM_BAD_ARG, "%u players: too many for one launch", n);
  if (rdoom_status s = rdoom::check_device(&src, the_noun)) return s;
  if (things->n_levels != src.n_levels)
    return rdoom::fail(RDOOM_BAD_ARG, "a thing set of %u levels for a %s of %u", things->n_levels, noun, src.n_levels);
  if (things->device != src.device)
    return rdoom::fail(RDOOM_BAD_ARG, "the thing set lives on device %d, the %s on device %d", things->device, noun, src.device);
  if ((d_collected || d_visible_out || d_touched_out) && stride < things->words)
    return rdoom::fail(RDOOM_BAD_ARG, "a stride of %u words is smaller than the %u a row of the thing set's bits takes", stride, things->words);
  if (rdoom_status s = rdoom::check_offsets(d_offsets, n_objects, src.game_objects, noun)) return s;
  if (d_offsets && n_objects <= things->max_object_id)
    return rdoom::fail(RDOOM_BAD_ARG, "n_objects %u is not above the thing set's largest object_id %u", n_objects, things->max_object_id);
  a = ThingSenseArgs{d_states,      d_offsets, things->d_things.get(), d_collected,      d_visible_out,        d_touched_out,
                     d_nearest_out, d_new_out, n_objects,        stride,            params->max_range,    params->cos_half_fov,
                     params->touch_radius, params->touch_below, params->touch_above, params->collect_mask};
  return RDOOM_OK;
}

LineTable line_table(const rdoom::MapDevice &d) { return LineTable{d.seg.get(), d.heights.get(), d.ids.get(), d.flags.get()}; }

}  // namespace

extern "C" {

rdoom_status rdoom_thingset_create(const rdoom_thing *const *things, const uint32_t *counts, uint32_t n_levels, rdoom_thingset **out) {
  if (!out) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  *out = nullptr;
  if (!things || !counts || n_levels == 0) return rdoom::fail(RDOOM_BAD_ARG, "a thing set needs at least one level's table");
  return rdoom::guarded([&]() -> rdoom_status {
    std::vector<rdoom_thing> all;
    std::vector<uint2> levels;
    uint32_t most = 0, max_object_id = 0;
    for (uint32_t l = 0; l < n_levels; l++) {
      if (counts[l] > MAX_THINGS) return rdoom::fail(RDOOM_BAD_ARG, "level %u has %u things (at most %u)", l, counts[l], MAX_THINGS);
      if (counts[l] && !things[l]) return rdoom::fail(RDOOM_BAD_ARG, "level %u: %u things at a null pointer", l, counts[l]);
      levels.push_back(make_uint2((uint32_t)all.size(), counts[l]));
      most = counts[l] > most ? counts[l] : most;
      for (uint32_t i = 0; i < counts[l]; i++) {
        const rdoom_thing &t = things[l][i];
        if ((t.category & 0xFFu) > RDOOM_THING_UNKNOWN || (t.category & ~(0xFFu | RDOOM_THING_HANGING)))
          return rdoom::fail(RDOOM_BAD_ARG, "level %u, thing %u: category %#x", l, i, t.category);
        if (!is_finite(t.x) || !is_finite(t.z) || !is_finite(t.base) || !is_finite(t.radius) || t.radius < 0.0f)
          return rdoom::fail(RDOOM_BAD_ARG, "level %u, thing %u: x, z, base and radius must be finite and the radius >= 0", l, i);
        max_object_id = t.object_id > max_object_id ? t.object_id : max_object_id;
        all.push_back(t);
      }
    }
    if (all.size() > 0x7FFFFFFFu) return rdoom::fail(RDOOM_BAD_ARG, "%zu things in all: too many for one set", all.size());
    auto set = std::make_unique<rdoom_thingset>();
    HIP_TRY(hipGetDevice(&set->device));
    if (rdoom_status s = set->d_things.upload(all, rdoom::EMPTY_TABLE_BYTES)) return s;
    if (rdoom_status s = set->d_levels.upload(levels, rdoom::EMPTY_TABLE_BYTES)) return s;
    set->level0 = levels[0], set->n_levels = n_levels, set->max_object_id = max_object_id;
    set->words = most ? (most + 31u) / 32u : 1u;
    *out = set.release();
    return RDOOM_OK;
  });
}

void rdoom_thingset_destroy(rdoom_thingset *set) { delete set; }

rdoom_status rdoom_thingset_info(const rdoom_thingset *set, uint32_t *out_n_levels, uint32_t *out_words, uint32_t *out_max_object_id) {
  if (!set) return rdoom::fail(RDOOM_BAD_ARG, "null thing set");
  if (out_n_levels) *out_n_levels = set->n_levels;
  if (out_words) *out_words = set->words;
  if (out_max_object_id) *out_max_object_id = set->max_object_id;
  return RDOOM_OK;
}

rdoom_status rdoom_world_sense_things(const rdoom_world *w, const rdoom_thingset *things, const rdoom_player_state *d_states, uint32_t n,
                                      const float *d_object_offsets, uint32_t n_objects, const rdoom_thing_sense *params,
                                      uint32_t *d_collected, uint32_t *d_visible_out, uint32_t *d_touched_out, uint32_t stride,
                                      rdoom_thing_nearest *d_nearest_out, uint32_t *d_new_out, void *stream) {
  if (!w) return rdoom::fail(RDOOM_BAD_ARG, "null world");
  const rdoom::MapSource src = rdoom::map_source(w);
  ThingSenseArgs a;
  if (rdoom_status s = sense_args(src, "world", "the world", things, d_states, nullptr, false, n, d_object_offsets, n_objects, params,
                                  d_collected, d_visible_out, d_touched_out, stride, d_nearest_out, d_new_out, a))
    return s;
  if (!n) return RDOOM_OK;
  return rdoom::launch_checked(sense_things_kernel, dim3(n), dim3(THREADS), 0, stream, a, line_table(*src.map), things->level0,
                               src.map->n_lines);
}

rdoom_status rdoom_worldset_sense_things(const rdoom_worldset *set, const rdoom_thingset *things, const rdoom_player_state *d_states,
                                         const uint32_t *d_levels, uint32_t n, const float *d_object_offsets, uint32_t n_objects,
                                         const rdoom_thing_sense *params, uint32_t *d_collected, uint32_t *d_visible_out,
                                         uint32_t *d_touched_out, uint32_t stride, rdoom_thing_nearest *d_nearest_out, uint32_t *d_new_out,
                                         void *stream) {
  if (!set) return rdoom::fail(RDOOM_BAD_ARG, "null world set");
  const rdoom::MapSource src = rdoom::map_source(set);
  ThingSenseArgs a;
  if (rdoom_status s = sense_args(src, "world set", "the world set", things, d_states, d_levels, true, n, d_object_offsets, n_objects,
                                  params, d_collected, d_visible_out, d_touched_out, stride, d_nearest_out, d_new_out, a))
    return s;
  if (!n) return RDOOM_OK;
  return rdoom::launch_checked(worldset_sense_things_kernel, dim3(n), dim3(THREADS), 0, stream, a, line_table(*src.map),
                               (const uint2 *)src.map->levels.get(), (const uint2 *)things->d_levels.get(), d_levels, src.map->n_levels);
}

}  // extern "C"
