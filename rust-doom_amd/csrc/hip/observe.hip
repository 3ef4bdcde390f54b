// Reduced-size observations (rdoom_batch_resolve_observation): every fx x fy cell of a frame of the batch's last render as one
// element -- the exact mean of its RGB8 colours (interleaved or channel-first), the grey value of that mean's sums, or the smallest
// depth.  include/rdoom.h has the contract; a resolve pass that reduces before it stores, so that a policy's 160 x 100 input of a
// 640 x 400 render costs 1/16 of resolve_rgb's stores and no second pass over a full-size frame.
//
// A pixel's colour is resolve.hip's (PLAYPAL 0 where drawn, the clear colour where not), its depth planes.hip's (plane_record.hpp:
// the same device functions, so the same bits), and both are found by render_walk.hpp's walk: the quadrant table, the visibility
// words, then the fixup list.  The list is where this unit differs.  Outside described quadrants the main pass has read the list's
// pixels already.  Inside, a fix pixel changes its cell's sum or minimum, so a cell cannot be patched per pixel: observe_fix_kernel
// takes one fix item a thread and recomputes the item's WHOLE cell -- the pixels of the cell that are on the list (found by one walk
// over the list, which is short) from vis[o] / fb[o], the others from the table's record -- and stores it over what observe_kernel
// wrote.  Two items of one cell store the same bytes.
//
// fx, fy are 1, 2, 4 or 8, so a cell never straddles a 32 x 32 quadrant and the table entry is uniform for every cell of a wave.
// The decomposition is the walk's: a wave per quadrant, two lanes a row, 16 pixels a lane (one 16-byte index load), the palette
// staged once per workgroup in LDS.  Horizontal sums are lane-local (fx divides 16: the template parameter), vertical sums and
// minima combine the fy rows by __shfl_xor steps of 2, 4, 8 lanes (fy: a kernel argument).  The lane of a cell row's first pixel
// row stores the lane's cells as one contiguous run of the output row -- at fx = 8 the even lane takes the odd lane's two cells
// too, so a run is never shorter than 4 cells -- in dword stores where the run starts on a dword, in byte stores where not.
// Integer arithmetic only for the colours; no scratch; the only LDS is the palette.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "plane_record.hpp"
#include "render_walk.hpp"

#pragma clang fp contract(off)

namespace rdoom_dev {
namespace {

constexpr uint32_t CLEAR_WORD = RDOOM_CLEAR_R | (RDOOM_CLEAR_G << 8) | (RDOOM_CLEAR_B << 16);

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef u32x2 u32x2_a4 __attribute__((aligned(4)));  // 8-byte accesses at dword alignment, beside the walk's 16-byte ones

// what both kernels need of the frame and of the cells, in one kernel argument
struct ObsGeom {
  uint32_t first, count, groups_x, groups_per_frame, width, pitch, height, tiles_x, n_tiles, flags, cap;
  uint32_t lfy;     // log2 fy
  uint32_t ow, oh;  // cells per row, rows of cells
};

// ---- one cell ---------------------------------------------------------------------------------------------------------------
// lg = log2(fx * fy).  The contract's (2 S + n) / (2 n) and (77 S_r + 150 S_g + 29 S_b + 128 n) / (256 n), n a power of two.
__device__ __forceinline__ uint32_t cell_mean(uint32_t s, uint32_t lg) { return (2u * s + (1u << lg)) >> (lg + 1u); }

// the cell as one word: R | G << 8 | B << 16 of the means (both RGB8 layouts), or the grey byte
template <uint32_t FMT>
__device__ __forceinline__ uint32_t cell_word(uint32_t sr, uint32_t sg, uint32_t sb, uint32_t lg) {
  if (FMT == RDOOM_OBS_GRAY8) return (77u * sr + 150u * sg + 29u * sb + (128u << lg)) >> (8u + lg);
  return cell_mean(sr, lg) | (cell_mean(sg, lg) << 8) | (cell_mean(sb, lg) << 16);
}

__device__ __forceinline__ float depth_min(float d, float m) { return d < m ? d : m; }  // (a NaN is never taken)

// ---- stores -----------------------------------------------------------------------------------------------------------------
template <int NW>
__device__ __forceinline__ void store_words(uint32_t *d, const uint32_t (&w)[NW]) {
#pragma unroll
  for (int i = 0; i + 4 <= NW; i += 4) *reinterpret_cast<u32x4_a4 *>(d + i) = u32x4{w[i], w[i + 1], w[i + 2], w[i + 3]};
  constexpr int r = NW & ~3;
  if constexpr ((NW & 3) >= 2) *reinterpret_cast<u32x2_a4 *>(d + r) = u32x2{w[r], w[r + 1]};
  if constexpr ((NW & 1) != 0) d[NW - 1] = w[NW - 1];
}

// N bytes of a row, of which the first nv exist (the row ends there)
template <int N>
__device__ __forceinline__ void store_bytes(uint8_t *d, const uint32_t (&b)[N], uint32_t nv) {
  if constexpr (N >= 4) {
    if (nv >= (uint32_t)N && ((uintptr_t)d & 3u) == 0u) {
      uint32_t w[N / 4];
#pragma unroll
      for (int j = 0; j < N / 4; j++) w[j] = b[4 * j] | (b[4 * j + 1] << 8) | (b[4 * j + 2] << 16) | (b[4 * j + 3] << 24);
      store_words<N / 4>(reinterpret_cast<uint32_t *>(d), w);
      return;
    }
  }
#pragma unroll
  for (int i = 0; i < N; i++)
    if ((uint32_t)i < nv) d[i] = (uint8_t)b[i];
}

// NS cells of frame f (of the range), output row yo, from column cx0 on; cx0 < ow
template <uint32_t FMT, int NS>
__device__ __forceinline__ void store_cells(void *out, uint32_t f, uint32_t yo, uint32_t cx0, uint32_t ow, uint32_t oh,
                                            const uint32_t (&cw)[NS]) {
  const uint32_t nv = ow - cx0;
  if (FMT == RDOOM_OBS_DEPTH_MIN) {
    uint32_t *d = reinterpret_cast<uint32_t *>(out) + ((size_t)f * oh + yo) * ow + cx0;
    if (nv >= (uint32_t)NS) {
      store_words<NS>(d, cw);
    } else {
#pragma unroll
      for (int i = 0; i < NS; i++)
        if ((uint32_t)i < nv) d[i] = cw[i];
    }
  } else if (FMT == RDOOM_OBS_GRAY8) {
    store_bytes<NS>(reinterpret_cast<uint8_t *>(out) + ((size_t)f * oh + yo) * ow + cx0, cw, nv);
  } else if (FMT == RDOOM_OBS_RGB8_PLANAR) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
      uint32_t b[NS];
#pragma unroll
      for (int i = 0; i < NS; i++) b[i] = (cw[i] >> (8 * c)) & 0xFFu;
      store_bytes<NS>(reinterpret_cast<uint8_t *>(out) + (((size_t)f * 3u + c) * oh + yo) * ow + cx0, b, nv);
    }
  } else {  // RDOOM_OBS_RGB8
    uint32_t b[3 * NS];
#pragma unroll
    for (int i = 0; i < NS; i++) b[3 * i] = cw[i] & 0xFFu, b[3 * i + 1] = (cw[i] >> 8) & 0xFFu, b[3 * i + 2] = (cw[i] >> 16) & 0xFFu;
    store_bytes<3 * NS>(reinterpret_cast<uint8_t *>(out) + (((size_t)f * oh + yo) * ow + cx0) * 3u, b, nv * 3u);
  }
}

// ---- the main pass ----------------------------------------------------------------------------------------------------------
template <uint32_t FMT, int LFX, bool VIS16>
__global__ __launch_bounds__(256) void observe_kernel(const uint8_t *__restrict__ fb, const void *__restrict__ vis,
                                                      const uint32_t *__restrict__ qtab, const PoseConst *__restrict__ poses,
                                                      const uint32_t *__restrict__ palettes, const TriRec *__restrict__ recs,
                                                      void *__restrict__ out, ObsGeom g) {
  constexpr bool COLOUR = FMT != RDOOM_OBS_DEPTH_MIN;
  constexpr int FX = 1 << LFX, NC = 16 / FX;  // cells per lane
  constexpr int NS = LFX == 3 ? 4 : NC;       // cells per storing lane
  constexpr uint32_t NONE_ID = VisWord<VIS16>::none;
  __shared__ uint32_t pal[COLOUR ? 256 : 1];
  const WalkLane l = walk_lane(g.first, g.groups_x, g.groups_per_frame);
  const uint32_t f = l.f, pose = l.pose, lane = l.lane, qx = l.qx, x0 = l.x0;
  if (COLOUR) {
    pal[threadIdx.x] = palettes[(size_t)poses[pose].level * 256u + threadIdx.x];  // the pose's PLAYPAL 0, staged once
    __syncthreads();
  }
  const uint32_t width = g.width, height = g.height, pitch = g.pitch;
  if (qx * 32u >= width) return;  // (wave-uniform; no barrier follows)
  const size_t frame = (size_t)pitch * height;
  const uint8_t *pfb = fb + (size_t)pose * frame;
  const void *pvis = vis_of_pose<VIS16>(vis, pose, frame);
  const TriRec *prec = recs + (size_t)pose * g.cap;
  const LevelTables no_tables{};  // (depth reads none)
  const uint32_t lfy = g.lfy, lg = (uint32_t)LFX + lfy;
  for (uint32_t k = 0; k < WALK_QROWS; k++) {
    const uint32_t qy = l.gy * WALK_QROWS + k;
    if (qy * 32u >= height) break;
    const uint32_t ent = quadrant_entry(qtab, g.flags, pose, g.n_tiles, g.tiles_x, qx, qy);
    const bool described = ent != NONE;
    const uint32_t y = qy * 32u + (lane >> 1);
    // Every lane stays in step to the shuffles below.  A lane outside the frame loads nothing; what it and the pixels past the
    // row's end contribute goes to cells that hold a column >= width or a row >= height, and no such cell is stored.
    const bool inside = y < height && x0 < width, whole = x0 + 16u <= width;
    const uint32_t npx = inside ? min(width - x0, 16u) : 0u;
    const size_t o = (size_t)y * pitch + x0;
    uint32_t cw[NC];
    if (COLOUR) {
      u32x4 idx{0u, 0u, 0u, 0u};
      uint32_t drawn = described ? 0xFFFFu : 0u;  // bit i: pixel x0 + i shows a primitive
      if (inside && whole) {
        idx = *reinterpret_cast<const u32x4_a4 *>(pfb + o);
        if (!described) drawn = vis_run_drawn<VIS16>(pvis, o);
      } else if (inside) {  // the row's last pixels (a width that is not a multiple of 16)
#pragma unroll
        for (int i = 0; i < 16; i++) {
          if ((uint32_t)i < npx) {
            idx[i >> 2] |= (uint32_t)pfb[o + i] << (8 * (i & 3));
            if (!described) drawn |= (vis_word<VIS16>(pvis, o + i) != NONE_ID ? 1u : 0u) << i;
          }
        }
      }
      uint32_t srb[NC], sg[NC];  // S_r | S_b << 16 (a sum is at most 64 * 255), S_g
#pragma unroll
      for (int c = 0; c < NC; c++) {
        srb[c] = 0u, sg[c] = 0u;
#pragma unroll
        for (int j = 0; j < FX; j++) {
          const int i = c * FX + j;
          const uint32_t p = pal[(idx[i >> 2] >> (8 * (i & 3))) & 0xFFu];  // (looked up whether drawn or not: no branch per pixel)
          const uint32_t col = ((drawn >> i) & 1u) ? p : CLEAR_WORD;
          srb[c] += col & 0xFF00FFu, sg[c] += (col >> 8) & 0xFFu;
        }
      }
#pragma unroll
      for (uint32_t s = 0; s < 3; s++) {  // rows y ^ 1, then ^ 2, then ^ 4: lanes 2, 4, 8 apart
        if (s < lfy) {
#pragma unroll
          for (int c = 0; c < NC; c++) srb[c] += __shfl_xor(srb[c], 2 << s), sg[c] += __shfl_xor(sg[c], 2 << s);
        }
      }
#pragma unroll
      for (int c = 0; c < NC; c++) cw[c] = cell_word<FMT>(srb[c] & 0xFFFFu, sg[c], srb[c] >> 16, lg);
    } else {
      uint32_t d[16];
#pragma unroll
      for (int i = 0; i < 16; i++) d[i] = DEPTH_FAR;
      RecVal qrec{0.0f, 0.0f, 0.0f, 0u};
      if (described) {  // wave-uniform: the record's words by scalar loads
        const uint32_t rec = min((uint32_t)__builtin_amdgcn_readfirstlane((int)(ent & ENTRY_REC_MASK)), g.cap - 1u);
        qrec = fetch_record<RDOOM_PLANE_DEPTH>(prec, rec, no_tables);
      }
      if (inside) {
        const float py = (float)y + 0.5f;
        if (described) {
#pragma unroll
          for (int i = 0; i < 16; i++) d[i] = plane_value<RDOOM_PLANE_DEPTH>(qrec, (float)(x0 + i) + 0.5f, py);
        } else {
          uint32_t w[16];
          if (whole) {
            vis_run<VIS16>(pvis, o, w);
          } else {
#pragma unroll
            for (int i = 0; i < 16; i++) w[i] = (uint32_t)i < npx ? vis_word<VIS16>(pvis, o + i) : NONE_ID;
          }
          uint32_t prev = NONE_ID;  // neighbours mostly share a record: gathered only where the word changes (planes.hip)
          RecVal rv{0.0f, 0.0f, 0.0f, 0u};
#pragma unroll
          for (int i = 0; i < 16; i++) {
            if (w[i] != NONE_ID && w[i] != prev) {
              rv = fetch_record<RDOOM_PLANE_DEPTH>(prec, min(w[i], g.cap - 1u), no_tables);
              prev = w[i];
            }
            d[i] = w[i] == NONE_ID ? DEPTH_FAR : plane_value<RDOOM_PLANE_DEPTH>(rv, (float)(x0 + i) + 0.5f, py);
          }
        }
      }
      float m[NC];
#pragma unroll
      for (int c = 0; c < NC; c++) {
        m[c] = __uint_as_float(DEPTH_FAR);
#pragma unroll
        for (int j = 0; j < FX; j++) m[c] = depth_min(__uint_as_float(d[c * FX + j]), m[c]);
      }
#pragma unroll
      for (uint32_t s = 0; s < 3; s++) {
        if (s < lfy) {
#pragma unroll
          for (int c = 0; c < NC; c++) m[c] = depth_min(__shfl_xor(m[c], 2 << s), m[c]);
        }
      }
#pragma unroll
      for (int c = 0; c < NC; c++) cw[c] = __float_as_uint(m[c]);
    }
    uint32_t cs[NS];
    if constexpr (LFX == 3) {  // two cells a lane: the even lane stores the row's four
      cs[0] = cw[0], cs[1] = cw[1], cs[2] = __shfl_xor(cw[0], 1), cs[3] = __shfl_xor(cw[1], 1);
    } else {
#pragma unroll
      for (int c = 0; c < NS; c++) cs[c] = cw[c];
    }
    const uint32_t cy = y >> lfy, cx0 = x0 >> LFX;
    const bool first_row = ((lane >> 1) & ((1u << lfy) - 1u)) == 0u && (LFX != 3 || (lane & 1u) == 0u);
    if (first_row && cy < g.oh && cx0 < g.ow)
      store_cells<FMT, NS>(out, f, (g.flags & WF_TOP_DOWN) ? g.oh - 1u - cy : cy, cx0, g.ow, g.oh, cs);
  }
}

// ---- the cells of the fixup list -------------------------------------------------------------------------------------------
// One fix item a thread: its whole cell again, the cell's pixels that are on the list from vis[o] / fb[o].  Runs after
// observe_kernel on the same stream.
template <uint32_t FMT, bool VIS16>
__global__ __launch_bounds__(256) void observe_fix_kernel(const uint8_t *__restrict__ fb, const void *__restrict__ vis,
                                                          const uint32_t *__restrict__ qtab, const PoseConst *__restrict__ poses,
                                                          const uint32_t *__restrict__ palettes, const TriRec *__restrict__ recs,
                                                          const uint32_t *__restrict__ fix_count, const uint2 *__restrict__ fix_list,
                                                          uint32_t fix_cap, void *__restrict__ out, ObsGeom g, uint32_t lfx) {
  constexpr bool COLOUR = FMT != RDOOM_OBS_DEPTH_MIN;
  constexpr uint32_t NONE_ID = VisWord<VIS16>::none;
  const uint32_t lfy = g.lfy, lg = lfx + lfy, fx = 1u << lfx, fy = 1u << lfy, pitch = g.pitch;
  const LevelTables no_tables{};  // (depth reads none)
  walk_fix_list<VIS16>(vis, fix_count, fix_list, fix_cap, g.first, g.count, g.width, pitch, g.height,
                       [&](uint32_t pose, uint32_t x, uint32_t y, uint32_t, bool) {
    const uint32_t cx = x >> lfx, cy = y >> lfy;
    if (cx >= g.ow || cy >= g.oh) return;  // a leftover column or row: in no cell
    const uint32_t ent = quadrant_entry(qtab, g.flags, pose, g.n_tiles, g.tiles_x, x >> 5, y >> 5);
    const bool described = ent != NONE;
    const uint32_t base = (cy << lfy) * pitch + (cx << lfx);  // the cell's first pixel
    // bit r * fx + c: the pixel's record is in vis[o].  Outside described quadrants that is every pixel; inside, those on the list.
    uint64_t from_vis = ~0ull;
    if (described) {
      from_vis = 1ull << ((y - (cy << lfy)) * fx + (x - (cx << lfx)));
      if (lg != 0u) {
        const uint32_t total = *fix_count;  // (within fix_cap: the walk is under way)
        for (uint32_t j = 0; j < total; j++) {
          const uint2 other = fix_list[j];
          const uint32_t dd = other.y - base;  // (an item before the cell wraps to a large number)
          if (other.x != pose || dd > (fy - 1u) * pitch + fx - 1u) continue;
          const uint32_t r = dd / pitch, c = dd - r * pitch;
          if (c < fx) from_vis |= 1ull << (r * fx + c);
        }
      }
    }
    const size_t po = (size_t)pose * pitch * g.height + base;
    const TriRec *prec = recs + (size_t)pose * g.cap;
    uint32_t cs[1];
    if (COLOUR) {
      const uint32_t *ppal = palettes + (size_t)poses[pose].level * 256u;
      uint32_t sr = 0u, sg = 0u, sb = 0u;
      for (uint32_t r = 0; r < fy; r++) {
        for (uint32_t c = 0; c < fx; c++) {
          const size_t o = po + (size_t)r * pitch + c;
          bool drawn = true;
          if ((from_vis >> (r * fx + c)) & 1ull) drawn = vis_word<VIS16>(vis, o) != NONE_ID;
          const uint32_t col = drawn ? ppal[fb[o]] : CLEAR_WORD;
          sr += col & 0xFFu, sg += (col >> 8) & 0xFFu, sb += (col >> 16) & 0xFFu;
        }
      }
      cs[0] = cell_word<FMT>(sr, sg, sb, lg);
    } else {
      RecVal qrec{0.0f, 0.0f, 0.0f, 0u};
      if (described) qrec = fetch_record<RDOOM_PLANE_DEPTH>(prec, min(ent & ENTRY_REC_MASK, g.cap - 1u), no_tables);
      float m = __uint_as_float(DEPTH_FAR);
      for (uint32_t r = 0; r < fy; r++) {
        for (uint32_t c = 0; c < fx; c++) {
          const float px = (float)((cx << lfx) + c) + 0.5f, py = (float)((cy << lfy) + r) + 0.5f;
          uint32_t d = plane_value<RDOOM_PLANE_DEPTH>(qrec, px, py);
          if ((from_vis >> (r * fx + c)) & 1ull) {
            const uint32_t w = vis_word<VIS16>(vis, po + (size_t)r * pitch + c);
            d = DEPTH_FAR;
            if (w != NONE_ID) d = plane_value<RDOOM_PLANE_DEPTH>(fetch_record<RDOOM_PLANE_DEPTH>(prec, min(w, g.cap - 1u), no_tables), px, py);
          }
          m = depth_min(__uint_as_float(d), m);
        }
      }
      cs[0] = __float_as_uint(m);
    }
    store_cells<FMT, 1>(out, pose - g.first, (g.flags & WF_TOP_DOWN) ? g.oh - 1u - cy : cy, cx, g.ow, g.oh, cs);
  });
}

template <uint32_t FMT, int LFX, bool VIS16>
void launch_main(hipStream_t st, uint32_t grid, const ObserveArgs &a, const ObsGeom &g) {
  hipLaunchKernelGGL((observe_kernel<FMT, LFX, VIS16>), dim3(grid), dim3(256), 0, st, a.fb, a.vis, a.qtab, a.poses, a.palettes, a.recs,
                     a.out, g);
}

template <uint32_t FMT, bool VIS16>
void launch_pair(hipStream_t st, uint32_t grid, const ObserveArgs &a, const ObsGeom &g, uint32_t lfx) {
  switch (lfx) {
    case 0: launch_main<FMT, 0, VIS16>(st, grid, a, g); break;
    case 1: launch_main<FMT, 1, VIS16>(st, grid, a, g); break;
    case 2: launch_main<FMT, 2, VIS16>(st, grid, a, g); break;
    default: launch_main<FMT, 3, VIS16>(st, grid, a, g); break;
  }
  hipLaunchKernelGGL((observe_fix_kernel<FMT, VIS16>), dim3(64), dim3(256), 0, st, a.fb, a.vis, a.qtab, a.poses, a.palettes, a.recs,
                     a.fix_count, a.fix_list, a.fix_cap, a.out, g, lfx);
}

template <uint32_t FMT>
void launch_format(hipStream_t st, uint32_t grid, const ObserveArgs &a, const ObsGeom &g, uint32_t lfx) {
  a.vis16 ? launch_pair<FMT, true>(st, grid, a, g, lfx) : launch_pair<FMT, false>(st, grid, a, g, lfx);
}

// 1, 2, 4, 8 -> 0..3; anything else -> 4
uint32_t factor_log2(uint32_t v) { return v == 1u ? 0u : v == 2u ? 1u : v == 4u ? 2u : v == 8u ? 3u : 4u; }

}  // namespace

size_t observation_cell_bytes(uint32_t format) { return format == RDOOM_OBS_DEPTH_MIN ? 4u : format == RDOOM_OBS_GRAY8 ? 1u : 3u; }

rdoom_status launch_observe(hipStream_t st, const ObserveArgs &a) {
  if (a.count == 0) return RDOOM_OK;
  const uint32_t lfx = factor_log2(a.fx), lfy = factor_log2(a.fy);
  if (lfx > 3u || lfy > 3u) return rdoom::fail(RDOOM_BAD_ARG, "internal: observation factors %u x %u", a.fx, a.fy);
  if (a.format == RDOOM_OBS_DEPTH_MIN && a.cap == 0) return rdoom::fail(RDOOM_BAD_ARG, "internal: a batch without records");
  if ((a.width >> lfx) == 0 || (a.height >> lfy) == 0) return rdoom::fail(RDOOM_BAD_ARG, "internal: an observation without cells");
  WalkLaunch wl;
  if (rdoom_status rs = walk_launch(a, "observations", false, &wl)) return rs;
  const ObsGeom g{a.first, a.count, wl.groups_x, wl.groups_per_frame, a.width, a.pitch, a.height, wl.tiles_x, wl.n_tiles, wl.flags, a.cap,
                  lfy, a.width >> lfx, a.height >> lfy};
  const uint32_t grid = wl.grid;
  switch (a.format) {
    case RDOOM_OBS_RGB8: launch_format<RDOOM_OBS_RGB8>(st, grid, a, g, lfx); break;
    case RDOOM_OBS_RGB8_PLANAR: launch_format<RDOOM_OBS_RGB8_PLANAR>(st, grid, a, g, lfx); break;
    case RDOOM_OBS_GRAY8: launch_format<RDOOM_OBS_GRAY8>(st, grid, a, g, lfx); break;
    case RDOOM_OBS_DEPTH_MIN: launch_format<RDOOM_OBS_DEPTH_MIN>(st, grid, a, g, lfx); break;
    default: return rdoom::fail(RDOOM_BAD_ARG, "unknown observation format %u", a.format);
  }
  HIP_TRY(hipGetLastError());
  return RDOOM_OK;
}

}  // namespace rdoom_dev
