// Things in the frame (include/rdoom_frame_things.h has the contracts).
//
// 1. The thing plane of a batch's last render (rdoom_batch_resolve_thing_plane): per pixel the thing of the winning decor triangle,
//    -1 elsewhere.  planes.hip's resolve pass with another value: the winning record is found the same way -- the quadrant table
//    first (a described quadrant's record by scalar loads, no visibility word read), then the visibility words with a gather only
//    where the word changes along a lane's run of 16 pixels, then the fixup list -- and what a record gives is its flags word: the
//    kind, and for decor the primitive id, whose word in DeviceLevelView::tri_thing is the element.  That second load is made for a
//    decor record only.  A wave resolves one 32 x 32 quadrant, two lanes a row; no LDS, no scratch.
//
// 2. rdoom_frame_things: per frame and thing the pixel count, the box and the smallest depth of an id plane, and a row of bits.
//    Three launches in stream order: the table's empty records; the reduction; the bit rows from the finished counts.  In the
//    reduction a workgroup takes a band of rows of one frame, a wave a row at a time, a lane four ids (16 bytes at dword alignment;
//    the last ids of a row one by one).  A wave none of whose lanes holds an id in range moves on at once.  Otherwise a lane folds
//    equal neighbouring ids of its four into runs and adds every run to a 64-slot table in LDS keyed by the id (open addressing,
//    LDS integer atomics); a run that finds the table full goes to the record in global memory directly.  At the end the table is
//    flushed with integer add / min / max atomics whose results nobody reads.  All of it commutes, so the result is the same
//    bits whatever the order.
#include <hip/hip_runtime.h>

#include "../common.hpp"
#include "kernels.hpp"
#include "rdoom_frame_things.h"

namespace rdoom_dev {
namespace {

constexpr uint32_t PLANE_QROWS = 4;  // quadrant rows per workgroup, as planes.hip
constexpr uint32_t PF_QTAB = 1u, PF_TOP_DOWN = 2u;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_a4 __attribute__((aligned(4)));  // 16-byte accesses at dword alignment (tight rows of any width)

// The element a record gives.  things: the pose's level's words of tri_thing (never null here: a handle without a table takes no
// kernel); ntri >= 1: the triangles of that level.  rec < cap (the callers clamp); the primitive id of a record is below ntri by
// construction (set-up writes tri - first_tri of a triangle of the pose's slice) and is clamped all the same: one word per triangle
// of the slice is all the table holds.  RDOOM_NO_THING is 0xFFFFFFFF: -1 as it stands.  With a wave-uniform rec both loads are scalar.
__device__ __forceinline__ uint32_t thing_of(const TriRec *__restrict__ prec, uint32_t rec, const uint32_t *__restrict__ things,
                                             uint32_t ntri) {
  const uint32_t rf = prec[rec].r.flags;
  if (((rf >> 27) & 3u) != RDOOM_KIND_DECOR) return NONE;
  return things[min(rf & 0xFFFFFFu, ntri - 1u)];
}

// grid and decomposition: plane_kernel's (planes.hip)
template <bool VIS16>
__global__ __launch_bounds__(256) void thing_plane_kernel(const void *__restrict__ vis, const uint32_t *__restrict__ qtab,
                                                          const PoseConst *__restrict__ poses, const TriRec *__restrict__ recs,
                                                          uint32_t cap, const uint32_t *__restrict__ tri_thing,
                                                          const LevelSlice *__restrict__ slices, uint32_t *__restrict__ out,
                                                          uint32_t first, uint32_t groups_x, uint32_t groups_per_frame,
                                                          uint32_t width, uint32_t pitch, uint32_t height, uint32_t tiles_x,
                                                          uint32_t n_tiles, uint32_t flags) {
  constexpr uint32_t NONE_ID = VIS16 ? 0xFFFFu : NONE;
  const uint32_t f = blockIdx.x / groups_per_frame, g = blockIdx.x - f * groups_per_frame;
  const uint32_t pose = first + f;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
  const uint32_t gy = g / groups_x, gx = g - gy * groups_x;
  const uint32_t qx = gx * 4u + wave;
  if (qx * 32u >= width) return;
  const uint32_t x0 = qx * 32u + (lane & 1u) * 16u;  // two lanes per row of the quadrant, 32 rows
  const size_t frame = (size_t)pitch * height;
  const uint16_t *pv16 = reinterpret_cast<const uint16_t *>(vis) + (size_t)pose * frame;
  const uint32_t *pv32 = reinterpret_cast<const uint32_t *>(vis) + (size_t)pose * frame;
  const TriRec *prec = recs + (size_t)pose * cap;
  const LevelSlice &sl = slices[poses[pose].level];  // (scalar loads: one pose per workgroup)
  const uint32_t *things = tri_thing + sl.first_tri;
  const uint32_t ntri = sl.ntri;
  for (uint32_t k = 0; k < PLANE_QROWS; k++) {
    const uint32_t qy = gy * PLANE_QROWS + k;
    if (qy * 32u >= height) break;
    // the table first: a described quadrant has no visibility words of this render.  pose < the batch's poses, the tile and the
    // quadrant inside the frame: the index is the one plane_kernel forms
    uint32_t ent = NONE;
    if (flags & PF_QTAB) ent = qtab[((size_t)pose * n_tiles + (qy >> 1) * tiles_x + (qx >> 1)) * 4u + (qy & 1u) * 2u + (qx & 1u)];
    const bool described = ent != NONE;
    uint32_t qv = NONE;
    if (described)  // wave-uniform: the record's flags and the thing's word by scalar loads
      qv = thing_of(prec, min((uint32_t)__builtin_amdgcn_readfirstlane((int)(ent & ENTRY_REC_MASK)), cap - 1u), things, ntri);
    const uint32_t y = qy * 32u + (lane >> 1);
    if (y >= height || x0 >= width) continue;
    const uint32_t yo = (flags & PF_TOP_DOWN) ? height - 1u - y : y;
    const size_t o = (size_t)y * pitch + x0;
    uint32_t *dst = out + ((size_t)f * height + yo) * width + x0;
    if (x0 + 16u <= width) {
      uint32_t c[16];
      if (described) {
#pragma unroll
        for (int i = 0; i < 16; i++) c[i] = qv;
      } else {
        uint32_t w[16];
        if (VIS16) {
          const u32x4 a = *reinterpret_cast<const u32x4_a4 *>(pv16 + o), b = *reinterpret_cast<const u32x4_a4 *>(pv16 + o + 8);
#pragma unroll
          for (int i = 0; i < 8; i++) {
            const uint32_t ww = i < 4 ? a[i] : b[i - 4];
            w[2 * i] = ww & 0xFFFFu, w[2 * i + 1] = ww >> 16;
          }
        } else {
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const u32x4 ww = *reinterpret_cast<const u32x4_a4 *>(pv32 + o + 4 * j);
#pragma unroll
            for (int i = 0; i < 4; i++) w[4 * j + i] = ww[i];
          }
        }
        uint32_t prev = NONE_ID, v = NONE;
#pragma unroll
        for (int i = 0; i < 16; i++) {
          if (w[i] != NONE_ID && w[i] != prev) {  // a new record in this run
            v = thing_of(prec, min(w[i], cap - 1u), things, ntri);
            prev = w[i];
          }
          c[i] = w[i] == NONE_ID ? NONE : v;
        }
      }
      u32x4_a4 *d = reinterpret_cast<u32x4_a4 *>(dst);  // rows of dwords are dword aligned whatever the width
#pragma unroll
      for (int q = 0; q < 4; q++) d[q] = u32x4{c[4 * q], c[4 * q + 1], c[4 * q + 2], c[4 * q + 3]};
    } else {  // the row's last pixels (a width that is not a multiple of 16)
      uint32_t prev = NONE_ID, v = NONE;
      for (uint32_t i = 0; i < width - x0; i++) {
        uint32_t e = NONE;
        if (described) {
          e = qv;
        } else {
          const uint32_t w = VIS16 ? (uint32_t)pv16[o + i] : pv32[o + i];
          if (w != NONE_ID) {
            if (w != prev) v = thing_of(prec, min(w, cap - 1u), things, ntri), prev = w;
            e = v;
          }
        }
        dst[i] = e;
      }
    }
  }
}

// The pixels fixup_kernel re-resolved (its final record is in vis[o]), for the frames in range: plane_fix_kernel's walk.
template <bool VIS16>
__global__ __launch_bounds__(256) void thing_plane_fix_kernel(const void *__restrict__ vis, const PoseConst *__restrict__ poses,
                                                              const TriRec *__restrict__ recs, uint32_t cap,
                                                              const uint32_t *__restrict__ tri_thing,
                                                              const LevelSlice *__restrict__ slices,
                                                              const uint32_t *__restrict__ fix_count, const uint2 *__restrict__ fix_list,
                                                              uint32_t fix_cap, uint32_t *__restrict__ out, uint32_t first, uint32_t count,
                                                              uint32_t width, uint32_t pitch, uint32_t height, uint32_t flags) {
  const uint32_t total = *fix_count;
  if (total > fix_cap) return;  // fixup_kernel did not run: the render's status says so (device_flags)
  for (uint32_t item = blockIdx.x * 256u + threadIdx.x; item < total; item += gridDim.x * 256u) {
    const uint2 it = fix_list[item];  // (pose, row * pitch + column)
    if (it.x - first >= count) continue;  // so it.x is a pose of the range, below the batch's poses
    const uint32_t y = it.y / pitch, x = it.y - y * pitch;
    if (x >= width || y >= height) continue;
    const size_t o = (size_t)it.x * pitch * height + it.y;
    const uint32_t w = VIS16 ? (uint32_t)reinterpret_cast<const uint16_t *>(vis)[o] : reinterpret_cast<const uint32_t *>(vis)[o];
    uint32_t v = NONE;
    if (w != (VIS16 ? 0xFFFFu : NONE)) {
      const LevelSlice &sl = slices[poses[it.x].level];
      v = thing_of(recs + (size_t)it.x * cap, min(w, cap - 1u), tri_thing + sl.first_tri, sl.ntri);
    }
    const uint32_t yo = (flags & PF_TOP_DOWN) ? height - 1u - y : y;
    out[((size_t)(it.x - first) * height + yo) * width + x] = v;
  }
}

template <bool VIS16>
void launch_thing_pair(hipStream_t st, uint32_t grid, const ThingPlaneArgs &a, uint32_t groups_x, uint32_t groups_per_frame,
                       uint32_t tiles_x, uint32_t n_tiles, uint32_t flags) {
  hipLaunchKernelGGL((thing_plane_kernel<VIS16>), dim3(grid), dim3(256), 0, st, a.vis, a.qtab, a.poses, a.recs, a.cap, a.tri_thing,
                     a.slices, (uint32_t *)a.out, a.first, groups_x, groups_per_frame, (uint32_t)a.width, (uint32_t)a.pitch,
                     (uint32_t)a.height, tiles_x, n_tiles, flags);
  hipLaunchKernelGGL((thing_plane_fix_kernel<VIS16>), dim3(64), dim3(256), 0, st, a.vis, a.poses, a.recs, a.cap, a.tri_thing, a.slices,
                     a.fix_count, a.fix_list, a.fix_cap, (uint32_t *)a.out, a.first, a.count, (uint32_t)a.width, (uint32_t)a.pitch,
                     (uint32_t)a.height, flags);
}

// ---- rdoom_frame_things ---------------------------------------------------------------------------------------------------------
constexpr uint32_t FT_THREADS = 256, FT_BAND = 16;  // rows of a frame per workgroup: four per wave
constexpr uint32_t FT_SLOTS = 64, FT_EMPTY = 0xFFFFFFFFu;  // (no id in range is 0xFFFFFFFF: max_things <= 2^20)
constexpr uint32_t FT_INF = 0x7F800000u;

struct FrameThingTable {  // 7 x 64 words = 1792 bytes of LDS
  uint32_t key[FT_SLOTS], count[FT_SLOTS];
  int32_t x0[FT_SLOTS], y0[FT_SLOTS], x1[FT_SLOTS], y1[FT_SLOTS];
  uint32_t depth[FT_SLOTS];
};

// a run's share of a record, by atomics whose results are not used.  p: any address space (LDS slot words or the global record)
__device__ __forceinline__ void merge(uint32_t *count, int32_t *x0, int32_t *y0, int32_t *x1, int32_t *y1, uint32_t *depth, uint32_t n,
                                      int32_t ax0, int32_t ay0, int32_t ax1, int32_t ay1, uint32_t d) {
  atomicAdd(count, n);
  atomicMin(x0, ax0);
  atomicMin(y0, ay0);
  atomicMax(x1, ax1);
  atomicMax(y1, ay1);
  if (d != FT_INF) atomicMin(depth, d);  // (bit patterns of non-negative floats order as the floats)
}

__device__ __forceinline__ void merge_global(rdoom_frame_thing *rec, uint32_t n, int32_t ax0, int32_t ay0, int32_t ax1, int32_t ay1,
                                             uint32_t d) {
  merge(&rec->count, &rec->x0, &rec->y0, &rec->x1, &rec->y1, reinterpret_cast<uint32_t *>(&rec->depth_min), n, ax0, ay0, ax1, ay1, d);
}

// one run of `n` pixels of thing id (< max_things, tested by the caller) in columns [xa, xb] of row y
__device__ __forceinline__ void add_run(FrameThingTable &t, rdoom_frame_thing *__restrict__ records, uint32_t id, uint32_t n, int32_t xa,
                                        int32_t xb, int32_t y, uint32_t d) {
  uint32_t s = (id * 0x9E3779B1u) >> 26;  // < 64
  for (uint32_t probe = 0; probe < FT_SLOTS; probe++, s = (s + 1u) & (FT_SLOTS - 1u)) {
    uint32_t k = __hip_atomic_load(&t.key[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (k == FT_EMPTY) {
      k = atomicCAS(&t.key[s], FT_EMPTY, id);  // (LDS, inside the workgroup: the slot is this id's from here on, or another's)
      if (k == FT_EMPTY) k = id;
    }
    if (k == id) {
      merge(&t.count[s], &t.x0[s], &t.y0[s], &t.x1[s], &t.y1[s], &t.depth[s], n, xa, y, xb, y, d);
      return;
    }
  }
  merge_global(records + id, n, xa, y, xb, y, d);  // the table is full of other ids
}

__global__ __launch_bounds__(256) void frame_things_init_kernel(rdoom_frame_thing *__restrict__ table, uint32_t total) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= total) return;  // total = n * max_things records, all of them the caller's
  uint32_t *w = reinterpret_cast<uint32_t *>(table + i);
  w[0] = 0u, w[1] = 0x7FFFFFFFu, w[2] = 0x7FFFFFFFu, w[3] = 0xFFFFFFFFu, w[4] = 0xFFFFFFFFu, w[5] = FT_INF;
}

// grid: n x bands workgroups; block f * bands + b takes rows [b * FT_BAND, min(height, (b + 1) * FT_BAND)) of frame f
__global__ __launch_bounds__(256) void frame_things_reduce_kernel(const uint32_t *__restrict__ ids, const uint32_t *__restrict__ depth,
                                                                  rdoom_frame_thing *__restrict__ table, uint32_t bands, uint32_t width,
                                                                  uint32_t height, uint32_t max_things) {
  __shared__ FrameThingTable t;
  const uint32_t f = blockIdx.x / bands, band = blockIdx.x - f * bands;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
  if (threadIdx.x < FT_SLOTS) {
    const uint32_t s = threadIdx.x;
    t.key[s] = FT_EMPTY, t.count[s] = 0u, t.x0[s] = 0x7FFFFFFF, t.y0[s] = 0x7FFFFFFF, t.x1[s] = -1, t.y1[s] = -1, t.depth[s] = FT_INF;
  }
  __syncthreads();
  rdoom_frame_thing *records = table + (size_t)f * max_things;
  const size_t frame = (size_t)f * width * height;  // width * height < 2^31, f < n: the frame's first element
  const uint32_t units = (width + 3u) >> 2, row_end = min(height, (band + 1u) * FT_BAND);
  for (uint32_t y = band * FT_BAND + wave; y < row_end; y += FT_THREADS / 64u) {
    const size_t row = frame + (size_t)y * width;
    for (uint32_t u = lane; u < units; u += 64u) {
      const uint32_t x = u * 4u, m = min(4u, width - x);  // x < width: m pixels of this row
      uint32_t v[4] = {FT_EMPTY, FT_EMPTY, FT_EMPTY, FT_EMPTY};
      if (m == 4u) {
        const u32x4 q = *reinterpret_cast<const u32x4_a4 *>(ids + row + x);
        v[0] = q[0], v[1] = q[1], v[2] = q[2], v[3] = q[3];
      } else {  // the row's last ids, one by one (constant indices: the four stay in registers)
#pragma unroll
        for (uint32_t i = 0; i < 3u; i++)
          if (i < m) v[i] = ids[row + x + i];
      }
      // an id below 0 is above max_things as a uint32: one compare, before any address is formed from it
      const bool any = (v[0] < max_things) | (v[1] < max_things) | (v[2] < max_things) | (v[3] < max_things);
      if (__ballot(any) == 0ull) continue;  // most of a frame shows no thing
      if (!any) continue;
      uint32_t d[4] = {FT_INF, FT_INF, FT_INF, FT_INF};
      if (depth) {
        if (m == 4u) {
          const u32x4 q = *reinterpret_cast<const u32x4_a4 *>(depth + row + x);
          d[0] = q[0], d[1] = q[1], d[2] = q[2], d[3] = q[3];
        } else {
#pragma unroll
          for (uint32_t i = 0; i < 3u; i++)
            if (i < m) d[i] = depth[row + x + i];
        }
      }
      uint32_t run_id = FT_EMPTY, run_n = 0u, run_x = 0u, run_d = FT_INF;
#pragma unroll
      for (uint32_t i = 0; i < 4u; i++) {
        const uint32_t id = v[i] < max_things ? v[i] : FT_EMPTY;  // (the pixels past the row's end are FT_EMPTY already)
        if (id != run_id) {
          if (run_id != FT_EMPTY) add_run(t, records, run_id, run_n, (int32_t)run_x, (int32_t)(x + i - 1u), (int32_t)y, run_d);
          run_id = id, run_n = 0u, run_x = x + i, run_d = FT_INF;
        }
        run_n++;
        run_d = min(run_d, d[i] < FT_INF ? d[i] : FT_INF);  // finite and not negative, or nothing
      }
      if (run_id != FT_EMPTY) add_run(t, records, run_id, run_n, (int32_t)run_x, (int32_t)(x + 3u), (int32_t)y, run_d);
    }
  }
  __syncthreads();
  if (threadIdx.x < FT_SLOTS) {
    const uint32_t s = threadIdx.x, k = t.key[s];
    if (k != FT_EMPTY && t.count[s]) merge_global(records + k, t.count[s], t.x0[s], t.y0[s], t.x1[s], t.y1[s], t.depth[s]);  // k < max_things
  }
}

// one thread per word of the bit rows: word w of frame f from the counts of things [32 w, 32 w + 32) below max_things
__global__ __launch_bounds__(256) void frame_things_bits_kernel(const rdoom_frame_thing *__restrict__ table, uint32_t *__restrict__ bits,
                                                                uint32_t total, uint32_t stride, uint32_t max_things, uint32_t min_pixels) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= total) return;  // total = n * stride words
  const uint32_t f = i / stride, w = i - f * stride;
  const rdoom_frame_thing *records = table + (size_t)f * max_things;
  uint32_t word = 0u;
  if (w < (max_things + 31u) / 32u) {  // (so 32 * w does not wrap)
    const uint32_t base = w * 32u, n = min(32u, max_things - base);
    for (uint32_t b = 0; b < n; b++) word |= (records[base + b].count >= min_pixels ? 1u : 0u) << b;
  }
  bits[i] = word;
}

}  // namespace

rdoom_status launch_thing_plane(hipStream_t st, const ThingPlaneArgs &a) {
  if (a.count == 0) return RDOOM_OK;
  const size_t elems = (size_t)a.count * (size_t)a.height * (size_t)a.width;
  if (!a.tri_thing) {  // a handle without a table: no pixel names a thing
    HIP_TRY(hipMemsetAsync(a.out, 0xFF, elems * sizeof(int32_t), st));
    return RDOOM_OK;
  }
  if (a.cap == 0) return rdoom::fail(RDOOM_BAD_ARG, "internal: a batch without records");
  const uint32_t tiles_x = ((uint32_t)a.width + TILE_W - 1u) / TILE_W, tiles_y = ((uint32_t)a.height + TILE_H - 1u) / TILE_H;
  const uint32_t groups_x = ((uint32_t)a.width + 127u) / 128u;
  const uint32_t row_groups = ((uint32_t)a.height + 32u * PLANE_QROWS - 1u) / (32u * PLANE_QROWS);
  const uint32_t groups_per_frame = groups_x * row_groups;
  const uint64_t grid = (uint64_t)groups_per_frame * a.count;
  if (grid > 0x7FFFFFFFull) return rdoom::fail(RDOOM_BAD_ARG, "thing planes of %u frames too large for one launch", a.count);
  const uint32_t flags = (a.use_qtab ? PF_QTAB : 0u) | (a.top_down ? PF_TOP_DOWN : 0u);
  a.vis16 ? launch_thing_pair<true>(st, (uint32_t)grid, a, groups_x, groups_per_frame, tiles_x, tiles_x * tiles_y, flags)
          : launch_thing_pair<false>(st, (uint32_t)grid, a, groups_x, groups_per_frame, tiles_x, tiles_x * tiles_y, flags);
  HIP_TRY(hipGetLastError());
  return RDOOM_OK;
}

}  // namespace rdoom_dev

using namespace rdoom_dev;

extern "C" {

rdoom_status rdoom_frame_things(const int32_t *d_ids, const float *d_depth, uint32_t n, uint32_t width, uint32_t height, uint32_t max_things,
                                uint32_t min_pixels, rdoom_frame_thing *d_table, uint32_t *d_bits, uint32_t stride, void *stream) {
  static_assert(sizeof(rdoom_frame_thing) == 24 && alignof(rdoom_frame_thing) == 4, "rdoom_frame_thing layout");
  if (min_pixels == 0) return rdoom::fail(RDOOM_BAD_ARG, "min_pixels 0: at least 1");
  if (max_things == 0 || max_things > (1u << 20)) return rdoom::fail(RDOOM_BAD_ARG, "max_things %u: 1 .. 2^20", max_things);
  if (width == 0 || height == 0) return rdoom::fail(RDOOM_BAD_ARG, "a %u x %u plane: width and height at least 1", width, height);
  if ((uint64_t)width * height >= (1ull << 31)) return rdoom::fail(RDOOM_BAD_ARG, "a %u x %u plane: width * height must be below 2^31", width, height);
  if (d_bits && stride == 0) return rdoom::fail(RDOOM_BAD_ARG, "stride 0 with bit rows given: at least 1");
  if (((uintptr_t)d_ids | (uintptr_t)d_depth | (uintptr_t)d_table | (uintptr_t)d_bits) & 3u)
    return rdoom::fail(RDOOM_BAD_ARG, "ids, depth, table and bits must be 4-byte aligned");
  if (!n) return RDOOM_OK;
  if (!d_ids || !d_table) return rdoom::fail(RDOOM_BAD_ARG, "null ids or table");
  const uint64_t records = (uint64_t)n * max_things, words = d_bits ? (uint64_t)n * stride : 0u;
  const uint32_t bands = (height + FT_BAND - 1u) / FT_BAND;
  if (records >= (1ull << 32) || words >= (1ull << 32) || (uint64_t)n * bands > 0x7FFFFFFFull)
    return rdoom::fail(RDOOM_BAD_ARG, "%u frames: too many records, words or rows for one call", n);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(frame_things_init_kernel, dim3((uint32_t)((records + 255u) / 256u)), dim3(256), 0, st, d_table, (uint32_t)records);
  hipLaunchKernelGGL(frame_things_reduce_kernel, dim3(n * bands), dim3(FT_THREADS), 0, st, reinterpret_cast<const uint32_t *>(d_ids),
                     reinterpret_cast<const uint32_t *>(d_depth), d_table, bands, width, height, max_things);
  if (d_bits)
    hipLaunchKernelGGL(frame_things_bits_kernel, dim3((uint32_t)((words + 255u) / 256u)), dim3(256), 0, st, d_table, d_bits, (uint32_t)words,
                       stride, max_things, min_pixels);
  HIP_TRY(hipGetLastError());
  return RDOOM_OK;
}

}  // extern "C"
