// Range-sensor rays that see things (include/rdoom_rays.h): rdoom_world_cast_rays_things and
// rdoom_worldset_cast_rays_things, a pass after the world cast.  The thing set is things.hip's (thingset.hpp), the ray is built
// with player_quat.hpp's functions in cast_rays' order, the pick of a level, the append and off() are world_shared.hpp's.
//
// Arithmetic: binary32, the contract's operations in the contract's order; the build passes -ffp-contract=off and HIP's division
// and square root are correctly rounded, so an IEEE host evaluating the header's expressions gets the same bits
// (tests/raythings_ref.py does).
//
// Shape: one 256-thread workgroup per player, as sense_player has it, so the state, the quaternion, the eye, the level slot and
// the row of offsets are the workgroup's.  The things are taken 256 at a time; thread t of pass k evaluates thing 256 k + t: the
// selection of the contract (select bit, hidden bit, category bit, R > 0) and the reach cull below.  The survivors are appended in
// index order (world_shared.hpp's append) to a static LDS list.  What a ray needs of a thing that does not depend on the ray is
// computed once, at the append, by the contract's own operations: cx, cz, cc = (cx * cx + cz * cz) - R * R, bottom, top; with the
// index that is 24 bytes an entry.  The list is folded over the rays when the next 256 things might not fit, and at the end.
// A fold takes the rays 64 at a time, lane l the ray 64 c + l; wave w takes entries w, w + 4, ... of the list (every lane of a
// wave reads the same entry: a broadcast read), the hit test and the minimum of the key bits(t) << 32 | index are selects, the
// four waves' keys meet in LDS and wave 0 settles the ray.  The key's minimum does not depend on the order or on where the list
// is cut.  Between folds the running fraction of a ray lives in d_frac_out, read and written by the one thread that owns the ray
// (plain loads and stores); the first fold reads d_frac_in.  A later fold holds higher indices only, so "replace when t < current,
// strictly" keeps the world on a tie and the lower index among equal t.  No atomics; every store is a plain vector store; every
// barrier is reached by every thread: the loops run on values every thread computes alike.
//
// The reach cull.  A hit needs a point of the ray's plan segment within R of the thing: in exact arithmetic
// |cx| <= |V.x| + R and |cz| <= |V.z| + R, hence both <= reach + R, reach the largest |V.x| + |V.z| of the player's finite rays.
// The contract's test is evaluated in binary32: its sums and products carry relative errors of a few 2^-24, and the one place
// where they are amplified is s = sqrtf(disc) near tangency, where h0 and h1 are off by at most about sqrt(8 * 2^-24) = 7e-4 of
// |c| / |V|; so a computed hit implies |c| <= 1.002 (|V| + R).  The cull drops a thing only when |cx| or |cz| is above
// 1.25 (reach + R), as computed -- a margin a hundred times that, which also covers the three roundings of the limit itself (one
// sum per ray, one sum and one product per thing).  It compares magnitudes, not squares: nothing under- or overflows in it, a limit
// that is +inf or a NaN keeps the thing, and with a == 0 (a vertical ray, or one whose squares underflow) the contract hits only
// with cc <= 0, which is |c| <= R.  The eye is finite where the cull runs: a player whose eye is not meets nothing.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../common.hpp"
#include "kernels.hpp"
#include "player_quat.hpp"
#include "rdoom_rays.h"
#include "thingset.hpp"
#include "world_shared.hpp"

#pragma clang fp contract(off)

namespace {

using rdoom_dev::append;
using rdoom_dev::Appended;
using rdoom_dev::live_height;
using rdoom_dev::player_eye;
using rdoom_dev::player_orientation;
using rdoom_dev::Quat;
using rdoom_dev::RayThingArgs;
using rdoom_dev::rotate;
using rdoom_dev::V3;
using rdoom_dev::with_level;

constexpr uint32_t WAVE = 64, THREADS = 256, WAVES = THREADS / WAVE;
constexpr uint32_t LIST_CAP = 512;      // things the LDS list holds: 512 x 24 bytes = 12 KiB
constexpr uint32_t FOLD_WAVES = WAVES;  // the waves that share a fold's list (1: wave 0 folds alone; DESIGN section 33 has the A/B)
constexpr uint64_t NO_KEY = ~0ull;      // above every key: t's bits are at most 1.0f's
constexpr float REACH_MARGIN = 1.25f;   // see "the reach cull" above

__device__ __forceinline__ bool finite(float v) { return __builtin_fabsf(v) < __builtin_inff(); }

// ray r of the player: vel = rotate(player, dir) * max_range, cast_ray's expression (world.hip)
__device__ __forceinline__ V3 ray_vel(const RayThingArgs &a, Quat player, uint32_t r) {
  const float *d = a.dirs + 3 * (size_t)r;
  const V3 dir = rotate(player, V3{d[0], d[1], d[2]});
  return V3{dir.x * a.max_range, dir.y * a.max_range, dir.z * a.max_range};
}

// player p against things [first, first + n_things) of the set, whose select bits are row `level` of a.select.  A slot outside
// the set comes here with no thing: its rays get current and -1
__device__ __forceinline__ void cast_player(const RayThingArgs &a, uint32_t p, uint32_t first, uint32_t n_things, uint32_t level) {
  __shared__ float4 list[LIST_CAP];    // cx, cz, cc, bottom
  __shared__ float2 tails[LIST_CAP];   // top, and the index as bits
  __shared__ uint64_t wave_key[FOLD_WAVES][WAVE];
  __shared__ uint32_t wave_kept[WAVES];
  __shared__ float wave_reach[WAVES];

  const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1), wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const rdoom_player_state *st = a.states + p;
  const Quat player = player_orientation(st->yaw, st->pitch);
  const V3 eye = player_eye(player, V3{st->pos[0], st->pos[1], st->pos[2]});
  if (!(finite(eye.x) && finite(eye.y) && finite(eye.z))) n_things = 0;  // the workgroup's: no ray of this player meets a thing

  // ---- the player's reach: the largest |V.x| + |V.z| of its finite rays
  float reach = 0.0f;
  if (n_things)
    for (uint32_t r = tid; r < a.n_rays; r += THREADS) {  // r + 256 < 2^32: n_rays <= 2^31
      const V3 v = ray_vel(a, player, r);
      const float plan = __builtin_fabsf(v.x) + __builtin_fabsf(v.z);
      reach = finite(v.x) && finite(v.y) && finite(v.z) && plan > reach ? plan : reach;
    }
  reach = rdoom_dev::wave_max(reach);
  if (lane == 0) wave_reach[wave] = reach;
  __syncthreads();
  reach = __builtin_fmaxf(__builtin_fmaxf(wave_reach[0], wave_reach[1]), __builtin_fmaxf(wave_reach[2], wave_reach[3]));

  const uint32_t *select = a.select ? a.select + (size_t)level * a.stride : nullptr;
  const uint32_t *hidden = a.hidden ? a.hidden + (size_t)p * a.stride : nullptr;
  const float *off = a.offsets ? a.offsets + (size_t)p * a.n_objects * 3 : nullptr;
  const uint4 *const record = reinterpret_cast<const uint4 *>(a.things + first);  // two words of 16 bytes a thing
  const size_t q0 = (size_t)p * a.n_rays;

  bool settled = false;  // a fold has run: the rays' running fractions are in frac_out.  The workgroup's
  uint32_t count = 0;
  uint32_t base = 0;
  do {
    const uint32_t t = base + tid;  // t < 2^20 + 256
    bool keep = false;
    float4 entry = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float2 tail = make_float2(0.0f, 0.0f);
    if (t < n_things) {
      const uint4 lo = record[2 * (size_t)t], hi = record[2 * (size_t)t + 1];
      const uint32_t chosen = select ? select[t >> 5] : ~0u, gone = hidden ? hidden[t >> 5] : 0u;  // word t / 32 < ceil(T / 32) <= stride
      const uint32_t category = hi.w & 0xFFu;  // the create call holds it to 0 .. 7
      const bool tried = ((chosen >> (t & 31u)) & 1u) && !((gone >> (t & 31u)) & 1u) && ((a.category_mask >> category) & 1u);
      const float x = __uint_as_float(lo.x), z = __uint_as_float(lo.y), radius = __uint_as_float(lo.w);
      const float R = radius + a.grow;
      float h = a.height[0];
#pragma unroll
      for (uint32_t k = 1; k < 8; k++) h = category == k ? a.height[k] : h;
      const float y = live_height(__uint_as_float(lo.z), hi.x, off, a.n_objects);
      const bool hanging = (hi.w & RDOOM_THING_HANGING) != 0;
      const float bottom = hanging ? y - h : y, top = hanging ? y : y + h;
      const float cx = eye.x - x, cz = eye.z - z;
      const float cc = (cx * cx + cz * cz) - R * R;
      const float limit = (reach + R) * REACH_MARGIN;
      const bool in_reach = !(__builtin_fabsf(cx) > limit) && !(__builtin_fabsf(cz) > limit);
      keep = tried && R > 0.0f && in_reach;
      entry = make_float4(cx, cz, cc, bottom);
      tail = make_float2(top, __uint_as_float(t));
    }
    const Appended kept = append<WAVES>(keep, lane, wave, wave_kept, count);
    if (keep) list[kept.slot] = entry, tails[kept.slot] = tail;  // count <= LIST_CAP - THREADS here, so kept.slot < LIST_CAP
    count += kept.total;
    base += THREADS;
    const bool fold = count > LIST_CAP - THREADS || base >= n_things;  // the next 256 might not fit, or there are none
    __syncthreads();
    if (fold && (count || !settled)) {
      for (uint32_t chunk = 0; chunk < a.n_rays; chunk += WAVE) {
        const uint32_t r = chunk + lane;
        const bool valid = r < a.n_rays;
        uint64_t key = NO_KEY;
        if (count && wave < FOLD_WAVES) {
          const V3 v = valid ? ray_vel(a, player, r) : V3{0.0f, 0.0f, 0.0f};
          const bool meets = finite(v.x) && finite(v.y) && finite(v.z) && !(v.x == 0.0f && v.y == 0.0f && v.z == 0.0f);
          const float aa = v.x * v.x + v.z * v.z;
          const bool slanted = aa > 0.0f, rising = v.y != 0.0f;
          if (meets)
            for (uint32_t e = wave; e < count; e += FOLD_WAVES) {
              const float4 s4 = list[e];
              const float b = s4.x * v.x + s4.y * v.z;
              const float disc = b * b - aa * s4.z;
              if (slanted ? disc >= 0.0f : s4.z <= 0.0f) {  // in plan
                const float2 s2 = tails[e];
                const float s = __builtin_sqrtf(disc);
                const float h0 = slanted ? (-b - s) / aa : -__builtin_inff(), h1 = slanted ? (-b + s) / aa : __builtin_inff();
                const float u0 = (s4.w - eye.y) / v.y, u1 = (s2.x - eye.y) / v.y;
                const float v0 = rising ? (u1 < u0 ? u1 : u0) : -__builtin_inff(), v1 = rising ? (u1 < u0 ? u0 : u1) : __builtin_inff();
                const bool in_height = rising || (eye.y >= s4.w && eye.y <= s2.x);
                float tt = h0 < v0 ? v0 : h0;
                tt = tt > 0.0f ? tt : 0.0f;
                const float end = v1 < h1 ? v1 : h1;
                const bool hit = in_height && tt <= end && tt <= 1.0f;
                const uint64_t k = (uint64_t)__float_as_uint(tt) << 32 | __float_as_uint(s2.y);
                key = hit && k < key ? k : key;
              }
            }
        }
        if (wave < FOLD_WAVES) wave_key[wave][lane] = key;
        __syncthreads();
        if (wave == 0 && valid) {
#pragma unroll
          for (uint32_t w = 1; w < FOLD_WAVES; w++) key = wave_key[w][lane] < key ? wave_key[w][lane] : key;
          const size_t q = q0 + r;
          const float current = settled ? a.frac_out[q] : (a.frac_in ? a.frac_in[q] : __builtin_inff());
          const float tt = __uint_as_float((uint32_t)(key >> 32));
          const bool replaces = key != NO_KEY && tt < current;
          if (replaces || !settled) {
            a.frac_out[q] = replaces ? tt : current;
            if (a.thing_out) a.thing_out[q] = replaces ? (int32_t)(uint32_t)key : -1;
          }
        }
        __syncthreads();  // before the next chunk's keys, and the next things, overwrite LDS
      }
      settled = true;
      count = 0;
    }
  } while (base < n_things);
}

__global__ __launch_bounds__(THREADS) void cast_rays_things_kernel(RayThingArgs a, uint2 things) {
  cast_player(a, blockIdx.x, things.x, things.y, 0u);
}

// the world set's: player p is in level level_of[p] of both sets; a slot outside them has no thing
__global__ __launch_bounds__(THREADS) void worldset_cast_rays_things_kernel(RayThingArgs a, const uint2 *__restrict__ thing_levels,
                                                                            const uint32_t *__restrict__ level_of, uint32_t n_levels) {
  const uint32_t p = blockIdx.x;
  const uint32_t lv = level_of[p];
  const bool in_set = lv < n_levels;
  uint32_t first = 0, n_things = 0;
  if (in_set)
    with_level(lv, [&](uint32_t slot) __attribute__((always_inline)) { first = thing_levels[slot].x, n_things = thing_levels[slot].y; });
  cast_player(a, p, first, n_things, in_set ? lv : 0u);
}

// what needs no handle, in the header's order
rdoom_status ray_things_free_args(const rdoom_thingset *things, const rdoom_player_state *d_states, const uint32_t *d_levels, bool needs_levels,
                                  uint32_t n, const float *d_dirs, uint32_t n_rays, float max_range, const rdoom_ray_things *params,
                                  const float *d_frac_in, const float *d_frac_out) {
  if (!things || !params || !d_dirs) return rdoom::fail(RDOOM_BAD_ARG, "null thing set, params or ray directions");
  if (n && (!d_states || !d_frac_out || (needs_levels && !d_levels)))
    return rdoom::fail(RDOOM_BAD_ARG, "null states, levels or fraction output with n = %u", n);
  if (rdoom_status s = rdoom::check_fan(n_rays, max_range)) return s;
  for (int c = 0; c < 8; c++)
    if (!(params->height[c] >= 0.0f)) return rdoom::fail(RDOOM_BAD_ARG, "height[%d] %g is not a number >= 0", c, (double)params->height[c]);
  if (!(params->grow >= 0.0f) || !std::isfinite(params->grow)) return rdoom::fail(RDOOM_BAD_ARG, "grow %g is not a finite number >= 0", (double)params->grow);
  if (params->flags) return rdoom::fail(RDOOM_BAD_ARG, "flags %#x: none is defined", params->flags);
  if (params->category_mask & ~0xFFu) return rdoom::fail(RDOOM_BAD_ARG, "category_mask %#x: there are eight categories", params->category_mask);
  if ((uint64_t)n * n_rays > 0x80000000ull) return rdoom::fail(RDOOM_BAD_ARG, "%u players x %u rays: too many for one launch", n, n_rays);
  const uint64_t bytes = (uint64_t)n * n_rays * 4u, x = (uintptr_t)d_frac_in, y = (uintptr_t)d_frac_out;
  if (d_frac_in && d_frac_out && x != y && (unsigned __int128)x < (unsigned __int128)y + bytes && (unsigned __int128)y < (unsigned __int128)x + bytes)
    return rdoom::fail(RDOOM_BAD_ARG, "d_frac_in and d_frac_out overlap in part: only the very same pointer is in place");
  return RDOOM_OK;
}

// what reads the handle and then the thing set; the kernel's arguments.  noun: "world" or "world set"
rdoom_status ray_things_args(const rdoom::MapSource &src, const char *noun, const char *the_noun, const rdoom_thingset *things,
                             const rdoom_player_state *d_states, const float *d_dirs, uint32_t n_rays, float max_range, const float *d_offsets,
                             uint32_t n_objects, const rdoom_ray_things *params, const uint32_t *d_select, const uint32_t *d_hidden,
                             uint32_t stride, const float *d_frac_in, float *d_frac_out, int32_t *d_thing_out, RayThingArgs &a) {
  if (rdoom_status s = rdoom::check_device(&src, the_noun)) return s;
  if (things->n_levels != src.n_levels)
    return rdoom::fail(RDOOM_BAD_ARG, "a thing set of %u levels for a %s of %u", things->n_levels, noun, src.n_levels);
  if (things->device != src.device)
    return rdoom::fail(RDOOM_BAD_ARG, "the thing set lives on device %d, the %s on device %d", things->device, noun, src.device);
  if ((d_select || d_hidden) && stride < things->words)
    return rdoom::fail(RDOOM_BAD_ARG, "a stride of %u words is smaller than the %u a row of the thing set's bits takes", stride, things->words);
  if (rdoom_status s = rdoom::check_offsets(d_offsets, n_objects, src.game_objects, noun)) return s;
  if (d_offsets && n_objects <= things->max_object_id)
    return rdoom::fail(RDOOM_BAD_ARG, "n_objects %u is not above the thing set's largest object_id %u", n_objects, things->max_object_id);
  a = RayThingArgs{d_states, d_dirs,   d_offsets, things->d_things.get(), d_select,  d_hidden, d_frac_in, d_frac_out, d_thing_out,
                   n_rays,   n_objects, stride,    params->category_mask,  max_range, params->grow, {}};
  for (int c = 0; c < 8; c++) a.height[c] = params->height[c];
  return RDOOM_OK;
}

}  // namespace

static_assert(sizeof(rdoom_ray_things) == 44 && sizeof(rdoom_thing) == 32, "ABI sizes");

extern "C" {

rdoom_status rdoom_world_cast_rays_things(const rdoom_world *w, const rdoom_thingset *things, const rdoom_player_state *d_states, uint32_t n,
                                          const float *d_dirs, uint32_t n_rays, float max_range, const float *d_object_offsets,
                                          uint32_t n_objects, const rdoom_ray_things *params, const uint32_t *d_select,
                                          const uint32_t *d_hidden, uint32_t stride, const float *d_frac_in, float *d_frac_out,
                                          int32_t *d_thing_out, void *stream) {
  if (rdoom_status s = ray_things_free_args(things, d_states, nullptr, false, n, d_dirs, n_rays, max_range, params, d_frac_in, d_frac_out)) return s;
  if (!w) return rdoom::fail(RDOOM_BAD_ARG, "null world");
  const rdoom::MapSource src = rdoom::map_source(w);
  RayThingArgs a;
  if (rdoom_status s = ray_things_args(src, "world", "the world", things, d_states, d_dirs, n_rays, max_range, d_object_offsets, n_objects, params,
                                       d_select, d_hidden, stride, d_frac_in, d_frac_out, d_thing_out, a))
    return s;
  if (!n) return RDOOM_OK;
  return rdoom::launch_checked(cast_rays_things_kernel, dim3(n), dim3(THREADS), 0, stream, a, things->level0);
}

rdoom_status rdoom_worldset_cast_rays_things(const rdoom_worldset *set, const rdoom_thingset *things, const rdoom_player_state *d_states,
                                             const uint32_t *d_levels, uint32_t n, const float *d_dirs, uint32_t n_rays, float max_range,
                                             const float *d_object_offsets, uint32_t n_objects, const rdoom_ray_things *params,
                                             const uint32_t *d_select, const uint32_t *d_hidden, uint32_t stride, const float *d_frac_in,
                                             float *d_frac_out, int32_t *d_thing_out, void *stream) {
  if (rdoom_status s = ray_things_free_args(things, d_states, d_levels, true, n, d_dirs, n_rays, max_range, params, d_frac_in, d_frac_out)) return s;
  if (!set) return rdoom::fail(RDOOM_BAD_ARG, "null world set");
  const rdoom::MapSource src = rdoom::map_source(set);
  RayThingArgs a;
  if (rdoom_status s = ray_things_args(src, "world set", "the world set", things, d_states, d_dirs, n_rays, max_range, d_object_offsets, n_objects,
                                       params, d_select, d_hidden, stride, d_frac_in, d_frac_out, d_thing_out, a))
    return s;
  if (!n) return RDOOM_OK;
  return rdoom::launch_checked(worldset_cast_rays_things_kernel, dim3(n), dim3(THREADS), 0, stream, a, (const uint2 *)things->d_levels.get(),
                               d_levels, src.map->n_levels);
}

}  // extern "C"
