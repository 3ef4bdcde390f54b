// Things in the frame (include/rdoom_frame_things.h has the contracts).
//
// rdoom_frame_things: per frame and thing the pixel count, the box and the smallest depth of an id plane, and a row of bits.  (The
// id plane itself, rdoom_batch_resolve_thing_plane's, is planes.hip's PLANE_THING.)
// Three launches in stream order: the table's empty records; the reduction; the bit rows from the finished counts.  In the
// reduction a workgroup takes a band of rows of one frame, a wave a row at a time, a lane four ids (16 bytes at dword alignment;
// the last ids of a row one by one).  A wave none of whose lanes holds an id in range moves on at once.  Otherwise a lane folds
// equal neighbouring ids of its four into runs and adds every run to a 64-slot table in LDS keyed by the id (open addressing,
// LDS integer atomics); a run that finds the table full goes to the record in global memory directly.  At the end the table is
// flushed with integer add / min / max atomics whose results nobody reads.  All of it commutes, so the result is the same
// bits whatever the order.
#include <hip/hip_runtime.h>

#include "../common.hpp"
#include "kernels.hpp"
#include "rdoom_frame_things.h"
#include "render_walk.hpp"  // u32x4_a4

namespace rdoom_dev {
namespace {

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
