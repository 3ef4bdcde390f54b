/* Things in the frame: a per-pixel thing plane of a batch's last render, and per-thing pixel counts, boxes and nearest depth of an
 * id plane.  A public header of its own beside rdoom.h, whose 135 functions stay as they are; the three entry
 * points below are exported by the same library.  The reference has no counterpart: this header is the authority.
 *
 * ---- the thing plane ----
 * rdoom_batch_resolve_thing_plane / rdoom_batch_read_thing_plane are a further plane of rdoom_batch_resolve_plane's family, with
 * an entry point of its own (rdoom_batch_resolve_plane goes on refusing every plane value it refused): int32, one element per
 * pixel of frames [first, first + count) of the batch's last render.  Rows are tight (width elements, no padding); row 0 is the
 * bottom row unless flags is RDOOM_RGB_TOP_DOWN.
 *
 * The element.  The pixel's winning fragment is the one rdoom_batch_resolve_plane names in RDOOM_PLANE_PRIMITIVE.  Where it is a
 * triangle of kind RDOOM_KIND_DECOR, of primitive id t in level L of its pose, and the level handle holds a thing table
 * (rdoom_level_set_decor_things), the element is that table's word for the quad of t -- the index of a thing in L's thing table, per
 * level in a level set -- unless the word is RDOOM_NO_THING.  Everywhere else the element is -1: flats, walls, sky, pixels nothing
 * was drawn to, decor of RDOOM_NO_THING, and every pixel of a handle without a table.  A thing a row of
 * rdoom_batch_set_hidden_things hid in the render is not drawn, so it is in no element.
 *
 * rdoom_batch_resolve_thing_plane writes count x height x width elements to d_out, device memory of the batch's device, 4-byte
 * aligned, asynchronously on `stream` behind the last render, as rdoom_batch_resolve_plane does; the checks of d_out are the ones
 * every resolve entry point makes.  rdoom_batch_read_thing_plane is synchronous, goes through the batch's bounded staging buffer,
 * writes host memory and reports the render's device flags, as rdoom_batch_read_plane does.  Errors (RDOOM_BAD_ARG): a bit of
 * flags other than RDOOM_RGB_TOP_DOWN; a NULL batch or output; nothing rendered yet; a frame range outside the last render; an
 * output that is not 4-byte aligned; (resolve) an output that is not device memory of the batch's device with room for the
 * frames.  count == 0 writes nothing.
 *
 * ---- what each frame shows of each thing ----
 * rdoom_frame_things reduces an id plane: n frames of height x width int32 ids, tight rows, whichever row order the caller made
 * them in (the thing plane above, or any other: RDOOM_PLANE_LABEL >> 4 widened to int32 gives the doors and lifts).  It needs no
 * batch and no handle.
 *
 * The record.  For frame f and thing i < max_things, over the pixels (x = column, y = row, as indexed in the plane) of frame f
 * with id == i: count is their number; x0, y0 their smallest column and row and x1, y1 their largest; depth_min the smallest
 * d_depth value (n x height x width binary32, rdoom_batch_resolve_plane's RDOOM_PLANE_DEPTH in the same row order) among those of
 * them whose bit pattern, read as uint32, is below 0x7F800000 -- finite and not negative, so +inf (sky, nothing drawn), NaN and
 * negative values never count -- and +inf when there is none or d_depth is NULL.  A thing with no pixel has count = 0, x0 = y0 =
 * INT32_MAX, x1 = y1 = -1, depth_min = +inf.  Record (f, i) is d_table[f * max_things + i].  An id below 0 or at or above
 * max_things is ignored; it is tested before any address is formed from it.
 *
 * The bits.  With d_bits, word w of row f, d_bits[f * stride + w], is written for every w < stride: bit i % 32 of word i / 32 is
 * set exactly when count_i >= min_pixels, for i < min(max_things, 32 * stride), and every other bit is 0 -- the layout of every
 * row of thing bits (rdoom_world_sense_things' d_collected, rdoom_batch_set_hidden_things' d_hidden), so a row can be OR-ed into
 * one of those as it stands.
 *
 * Every quantity is an integer or the bit pattern of a non-negative binary32, combined by add, min and max: the result does not
 * depend on the order in which pixels are visited, and is the same bits on every run.
 *
 * Limits, all RDOOM_BAD_ARG and all checked before anything is queued: min_pixels >= 1; 1 <= max_things <= 2^20; width, height
 * >= 1; width * height < 2^31; stride >= 1 when d_bits is given; (n > 0) a NULL d_ids or d_table; a pointer that is not 4-byte
 * aligned; n * max_things or n * stride at or above 2^32.  n == 0 is RDOOM_OK and queues nothing.  Outputs must not overlap inputs
 * or each other.  Nothing is assumed of a pointer beyond 4-byte alignment, and nothing outside records [0, n * max_things) and
 * words [0, n * stride) is written.
 *
 * Three launches, asynchronous on `stream`, ordered by the stream alone; nothing is allocated, nothing is copied and nothing
 * waits, so the call can be captured into a graph. */
#ifndef RDOOM_FRAME_THINGS_H
#define RDOOM_FRAME_THINGS_H

#include "rdoom.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rdoom_frame_thing {
  uint32_t count;         /* pixels whose id is this thing */
  int32_t x0, y0, x1, y1; /* inclusive box, in columns and rows of the plane as given */
  float depth_min;        /* smallest finite, non-negative depth among them; +inf when none */
} rdoom_frame_thing;      /* 24 bytes, 4-byte aligned */

rdoom_status rdoom_batch_resolve_thing_plane(rdoom_batch *batch, uint32_t first, uint32_t count, uint32_t flags, int32_t *d_out,
                                             void *stream);
rdoom_status rdoom_batch_read_thing_plane(rdoom_batch *batch, uint32_t first, uint32_t count, uint32_t flags, int32_t *out);
rdoom_status rdoom_frame_things(const int32_t *d_ids, const float *d_depth, uint32_t n, uint32_t width, uint32_t height,
                                uint32_t max_things, uint32_t min_pixels, rdoom_frame_thing *d_table, uint32_t *d_bits,
                                uint32_t stride, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RDOOM_FRAME_THINGS_H */
