/*
 * include/cairo_amd.h -- C ABI of libcairo_amd.so, the MI355X-native EVX-1
 * encode path.  Plain pointers and sizes only.
 *
 * Two layers:
 *
 *  1. The encode-path backend ("cairo_ctx_*").  It replaces the hot stages
 *     inside engine_encode_frame (reference encode.cpp:205-232): convert_image
 *     (convert.cpp:95-160), encode_slice (encode.cpp:165-203, with
 *     motion.cpp / transform.cpp / quantize.cpp / decode.cpp:15-144) and
 *     deblock_image_filter (deblock.cpp:277-284, fused into the row kernel).  Its outputs are exactly what
 *     the host entropy stage serialize_slice (serialize.cpp:319-340) consumes:
 *     the block table (evx_block_desc[], common.h:78-95, 16 B each) and the
 *     persistent quantized-coefficient planes (output_cache, common.h:108).
 *
 *  2. C wrappers of the drop-in C++ API (include/evx1.h), for FFI callers
 *     (ctypes): evx_encoder_* mirror evx1_encoder (reference evx1.h:66-94) and
 *     create_encoder / destroy_encoder (evx1.cpp:8-63); cairo_serialize_slice
 *     exposes the host entropy stage on its own.
 *
 * Status codes are evx_status values (reference base.h:150-172); a HIP
 * failure or a timed-out in-kernel wait maps to EVX_ERROR_HARDWAREFAIL (5).
 */
#ifndef CAIRO_AMD_H
#define CAIRO_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CAIRO_API __attribute__((visibility("default")))

/* Version of this C ABI.  It is bumped whenever an exported entry point
 * changes its signature or meaning; a caller built against one header checks
 * cairo_api_version() == CAIRO_AMD_API_VERSION at start-up.
 *   1  round 3: cairo_task_queues(hmb, frames, pool, ...)
 *   2  round 4: cairo_task_queues gains n_helpers and n_rows,
 *      cairo_group_check_queues gains hw_queues
 *   3  round 5: cairo_ctx_read_inter refuses stale (untagged) records
 *   4  pixel formats: cairo_frame_layout, cairo_ctx_submit_fmt,
 *      cairo_ctx_decode_frame_fmt, cairo_stream_submit_fmt, cairo_kat_convert,
 *      evx_encoder_set_input_format, evx_decoder_set_output_format
 *   4  (unchanged) per-frame metrics and kept reconstructions add entry points
 *      only: cairo_ctx_set_metrics, cairo_ctx_frame_metrics,
 *      cairo_ctx_fetch_recon[_planes], cairo_stream_frame_metrics,
 *      cairo_kat_metrics, evx_encoder_set_metrics / _last_metrics.  Nothing
 *      existing changes, so the version stays: detect them by their symbols.
 *   4  (unchanged) the scaled submit adds entry points only as well:
 *      cairo_source_size, cairo_scale_check, cairo_ctx_submit_scaled,
 *      cairo_stream_submit_scaled, cairo_kat_scale.
 *   4  (unchanged) cairo_table_check and cairo_desc_check are added.  The
 *      drop-in decoder refuses with an error some tables it used to decode
 *      (see cairo_table_check); every stream the reference encoder writes
 *      decodes as before.
 *   4  (unchanged) colour descriptions add entry points only:
 *      cairo_color_coefs, cairo_ctx_set_input_color, cairo_ctx_set_output_color,
 *      cairo_kat_convert_color, evx_encoder_set_input_color,
 *      evx_decoder_set_output_color.
 *   4  (unchanged) tensor frames add entry points only: cairo_tensor_size,
 *      cairo_tensor_check, cairo_tensor_host, cairo_kat_tensor,
 *      cairo_ctx_submit_tensor, cairo_stream_submit_tensor,
 *      cairo_ctx_decode_frame_tensor, cairo_ctx_fetch_recon_tensor,
 *      evx_encoder_set_input_tensor, evx_decoder_set_output_tensor.
 *   4  (unchanged) capture and 10-bit frames add values and one entry point
 *      only: the enumerators CAIRO_FMT_YUY2, CAIRO_FMT_UYVY and CAIRO_FMT_P010
 *      (8, 9, 10; values the entry points above refused before) and
 *      cairo_frame_fold.  Every call that took a format value takes them,
 *      except the scaled submit.  Nothing existing changes.
 *   4  (unchanged) the scaled tensor submit adds entry points only:
 *      cairo_tensor_scale_check, cairo_ctx_submit_tensor_scaled,
 *      cairo_stream_submit_tensor_scaled, cairo_kat_tensor_scale.
 *   4  (unchanged) cairo_kat_precode is added.  The host precode codes a value
 *      of -32768 as -32767 (31 bits, as the GPU precode always did) where it
 *      used to write 32 bits of a 33-bit code; no encoder produces the value.
 *   4  (unchanged) the target bitrate adds entry points only: cairo_rate_size,
 *      cairo_rate_state_size, cairo_rate_info_size, cairo_rate_estimate,
 *      cairo_rate_init, cairo_rate_step, cairo_ctx_set_rate,
 *      cairo_ctx_frame_rate, cairo_stream_frame_rate, cairo_kat_rate_observe.
 *      A context on which cairo_ctx_set_rate was never called behaves as
 *      before.
 *   4  (unchanged) cairo_kat_quant is added. */
#define CAIRO_AMD_API_VERSION 4
CAIRO_API int cairo_api_version(void);

typedef struct cairo_ctx cairo_ctx;

/* ---- pixel formats ---------------------------------------------------------
 * A frame is one contiguous buffer of 8-bit samples, `pitch` bytes from one
 * row to the next; pitch == 0 means tight (3*width for the RGB formats, width
 * for the YUV formats).  Widths and heights are even. */
#define CAIRO_FMT_RGB24 0  /* R,G,B bytes (today's format); pitch >= 3*width              */
#define CAIRO_FMT_BGR24 1  /* B,G,R bytes; pitch >= 3*width                               */
#define CAIRO_FMT_I420  2  /* Y: height rows of pitch bytes; then U: height/2 rows of     */
                           /* pitch/2 bytes; then V likewise. pitch even, >= width        */
#define CAIRO_FMT_NV12  3  /* Y: height rows of pitch bytes; then height/2 rows of pitch  */
                           /* bytes of interleaved U,V (U first). pitch >= width          */
/* BGR24 is RGB24 with the first and third byte swapped: same arithmetic, same
 * bits.  I420 and NV12 carry, by default, the codec's own colour space,
 * full-range BT.601 (JFIF): on input the internal planes are Y8 + 16, U8, V8
 * with no conversion; on output Y8 = clamp(Y - 16), U8 = clamp(U),
 * V8 = clamp(V), clamped to 0..255.  Limited-range and BT.709 frames are taken
 * and written under a colour description (below).
 * Pixels outside width x height are never read; on output the bytes of a row
 * beyond the image (the pitch padding) are never written. */

/* ---- capture and 10-bit frames ----------------------------
 * Frame layouts added after ABI 4 was pinned; 4..7 stay unassigned and refused. */
enum { CAIRO_FMT_YUY2 = 8, CAIRO_FMT_UYVY = 9, CAIRO_FMT_P010 = 10 };
/* What capture cards (packed 4:2:2) and 10-bit hardware decoders (P010) leave
 * in memory.  Widths and heights are even, as for every format.
 *   YUY2  one plane: height rows of pitch bytes; per pixel pair the four bytes
 *         Y0 U Y1 V.  Tight pitch 2*width, pitch*height bytes; pitch >= 2*width,
 *         any byte alignment of base and pitch.
 *   UYVY  the same with the bytes U Y0 V Y1.
 *   P010  16-bit little-endian words.  Y: height rows of pitch bytes, width
 *         words each; then height/2 rows of pitch bytes of interleaved U, V
 *         words (U first), width words each.  Tight pitch 2*width,
 *         pitch*height + pitch*(height/2) bytes; pitch even and >= 2*width.  A
 *         device frame's base must be 2-byte aligned (else
 *         EVX_ERROR_INVALID_ARGS).  The ten significant bits of a word are its
 *         high ten, v10 = word >> 6; the low six bits are ignored on input and
 *         written as zero on output.
 * The codec keeps 8-bit 4:2:0.  Each layout is defined by two pure
 * frame-to-frame maps onto NV12 of the same size, and everything else is what
 * the NV12 frame gets.
 *
 * fold (dir 0): a frame of the layout -> the NV12 frame (Y8 plane; U8, V8 at
 * (cx, cy), cx < width/2, cy < height/2).
 *   YUY2 / UYVY: Y8(x, y) = Y(x, y).  With U(cx, y) the U byte of pixel pair cx
 *     of row y:  U8(cx, cy) = (U(cx, 2cy) + U(cx, 2cy+1) + 1) >> 1, and V8
 *     likewise from V.  A 4:2:0 chroma sample lies between the two rows whose
 *     4:2:2 samples it replaces; the rule is their mean, halves rounded up (the
 *     rounding of the scaled submit's exact 2:1).
 *   P010: every sample, luma and chroma alike, is
 *     s8 = min((v10 + 2) >> 2, 255): round to nearest, halves up, clamped.
 *     Limited-range 10-bit code points land on their 8-bit ones (64 -> 16,
 *     940 -> 235, 960 -> 240).
 * unfold (dir 1): an NV12 frame -> the frame of the layout.
 *   YUY2 / UYVY: Y(x, y) = Y8(x, y); rows 2cy and 2cy+1 both get U8(cx, cy)
 *     and V8(cx, cy) for pair cx: the codec's rule that the luma sample at
 *     (x, y) uses the chroma sample at (x>>1, y>>1).
 *   P010: word = s8 << 8 for every sample.
 * fold(unfold(f)) == f for every NV12 frame f, in all three layouts (the mean
 * of two equal samples is that sample; ((s8 << 2) + 2) >> 2 == s8).
 *
 * Composition.  Input: submitting a frame of one of these layouts gives
 * exactly the bits of submitting fold(frame) as NV12 under the same input
 * colour description; the colour map runs on the folded 8-bit samples, and the
 * source side of the per-frame metrics is what the folded frame carries.
 * Output: cairo_ctx_decode_frame_fmt and cairo_ctx_fetch_recon write unfold of
 * the NV12 frame they would write under the same output colour description
 * (the colour map runs before the unfold).
 *
 * Refusals (EVX_ERROR_INVALID_ARGS).  cairo_scale_check,
 * cairo_ctx_submit_scaled and cairo_stream_submit_scaled refuse the three
 * layouts: the scale kernel walks planes of equally interleaved bytes, which
 * neither packed 4:2:2 nor 16-bit samples are; the refused submit takes no
 * ticket.  P010 with an odd pitch, or a P010 device frame at an odd address,
 * is refused.  Format values 4..7 and above 10 are refused as before. */

/* Buffer size and tight pitch of a frame (no device needed).
 * EVX_ERROR_INVALID_ARGS for an unknown format, an odd or zero size, a pitch
 * below the tight pitch, or an odd pitch for I420 or P010.  bytes /
 * tight_pitch may be NULL. */
CAIRO_API int cairo_frame_layout(int fmt, uint32_t width, uint32_t height, uint32_t pitch,
                                 uint64_t *bytes, uint32_t *tight_pitch);
/* fold and unfold on host buffers, with the per-sample code the kernels run
 * (no device needed).  fmt is CAIRO_FMT_YUY2, _UYVY or _P010; frame has row
 * pitch `pitch` and nv12 row pitch nv12_pitch (0: tight).  dir 0 reads frame
 * and writes the NV12 image bytes, dir 1 reads nv12 and writes the frame's
 * image bytes; pitch padding is never written.  EVX_ERROR_INVALID_ARGS for any
 * other format or a layout that cairo_frame_layout refuses. */
CAIRO_API int cairo_frame_fold(int dir, int fmt, uint32_t w, uint32_t h, uint32_t pitch, uint8_t *frame,
                               uint32_t nv12_pitch, uint8_t *nv12);

/* ---- colour descriptions ----------------------------------
 * A colour description is a pair (range, matrix): */
#define CAIRO_RANGE_FULL    0   /* Y, U, V 0..255 (today) */
#define CAIRO_RANGE_LIMITED 1   /* Y 16..235, chroma 16..240 nominal */
#define CAIRO_MATRIX_BT601  0   /* Kr = 0.299,  Kb = 0.114 (today) */
#define CAIRO_MATRIX_BT709  1   /* Kr = 0.2126, Kb = 0.0722 */
/* (FULL, BT601) is the codec's own space and the identity.  The description
 * applies only to the 8-bit samples of I420 and NV12 frames (and of the NV12
 * frame a YUY2, UYVY or P010 frame folds to or unfolds from, above).  RGB24
 * and BGR24 frames are taken and returned exactly as today whatever the
 * description is, so one launch and one ladder may mix them.
 *
 * Two maps are defined on the 8-bit sample triple:
 *   dir 0: described YUV to the codec's full-range BT.601 (input).
 *   dir 1: the codec's to described YUV (output).
 * A luma sample at (x, y) uses the chroma sample at (x>>1, y>>1), as the
 * codec's 4:2:0 does everywhere.  Chroma outputs never depend on luma.
 *
 * The real-valued matrix.  A(Kr, Kb), with Kg = 1 - Kr - Kb, is the RGB->YCbCr
 * matrix with rows
 *   [Kr, Kg, Kb]
 *   [-Kr, -Kg, 1-Kb] / (2(1-Kb))
 *   [1-Kr, -Kg, -Kb] / (2(1-Kr))
 * Then C_in(BT709) = A(601) A(709)^-1 and C_out(BT709) = A(709) A(601)^-1; both
 * have the shape [1 a b; 0 c d; 0 e f].  C(BT601) = I.  The range factors are
 * sy = 255/219 and sc = 255/224 for LIMITED, and 1 for FULL.  On input, column
 * 0 of C_in is multiplied by sy and columns 1 and 2 by sc, and oy = 16 is
 * subtracted from Y first.  On output, row 0 of C_out is divided by sy and rows
 * 1 and 2 by sc, and oy = 16 is added to Y.  (oy = 0 for FULL.)
 *
 * The integer coefficients.  k_ij = floor(2^14 c_ij + 1/2), computed in exact
 * rationals.  With d0 = Y8 - oy on input (d0 = Y8 on output), d1 = U8 - 128
 * and d2 = V8 - 128:
 *   in : Y' = clamp((k00 d0 + k01 d1 + k02 d2 + 2^13) >> 14)
 *   out: Y' = clamp((k00 d0 + k01 d1 + k02 d2 + (oy << 14) + 2^13) >> 14)
 *        U' = clamp((k11 d1 + k12 d2 + (128 << 14) + 2^13) >> 14)
 *        V' = clamp((k21 d1 + k22 d2 + (128 << 14) + 2^13) >> 14)
 * >> is arithmetic, there is one rounding per sample, and everything fits
 * int32.  The clamp is to 0..255.  Limited-range output is *not* clipped to
 * 16..235/240, and input bytes outside the nominal range are legal and go
 * through the same formula.
 *
 * How the maps compose with the existing paths.  Input: the internal planes
 * are the existing rule (Y8' + 16, U8', V8') applied to the mapped samples.
 * Output: the internal int16 samples are first clamped to 8 bits exactly as
 * the identity output does (clamp(Y - 16), clamp(U), clamp(V)), then mapped.
 * So for both directions the result equals the existing identity path composed
 * with a pure byte-frame map.
 *
 * The error bound.  Each coefficient is off by at most 2^-15, and |d0| <= 255,
 * |d1| and |d2| <= 128.  So every output is within 0.5 + 511/32768 of the
 * real-arithmetic value.  The clamp is 1-Lipschitz, so the bound survives it. */
/* The table the kernels use (host only, no device needed): k[9] row-major
 * (k00 k01 k02 | 0 k11 k12 | 0 k21 k22) and *offset = oy for dir 0 / 1.
 * EVX_ERROR_INVALID_ARGS for unknown values. */
CAIRO_API int cairo_color_coefs(int dir, int range, int matrix, int32_t k[9], int32_t *offset);
/* The description of the I420 / NV12 frames submitted from now on, through any
 * of cairo_ctx_submit_fmt, cairo_ctx_submit_scaled and cairo_stream_submit_*.
 * It is recorded per frame at submit, so it may change between submits with
 * frames in flight, and one launch may mix descriptions.  A scaled frame is
 * scaled first, on the samples as stored, then mapped: a scaled submit with a
 * description gives the bits of submitting the scaled frame with it.  Survives
 * cairo_ctx_reset; allowed for group members. */
CAIRO_API int cairo_ctx_set_input_color(cairo_ctx *ctx, int range, int matrix);
/* The description cairo_ctx_decode_frame_fmt and cairo_ctx_fetch_recon write
 * I420 / NV12 frames in from now on.  cairo_ctx_decode_frame,
 * cairo_ctx_fetch_recon_planes and the RGB formats are unchanged. */
CAIRO_API int cairo_ctx_set_output_color(cairo_ctx *ctx, int range, int matrix);

/* Outputs a context hands to the host entropy stage (cairo_ctx_set_outputs). */
#define CAIRO_OUT_COEF 1 /* the output_cache planes (default)                   */
#define CAIRO_OUT_FEED 2 /* the GPU entropy precode: the exact feed bits the    */
                         /* reference's coder consumes    */
#define CAIRO_FEED_NONE 0
#define CAIRO_FEED_VALID 1
#define CAIRO_FEED_OVERFLOW 2 /* a coefficient section exceeds the reference's   */
                              /* 32 Mbit feed stream: code it from the planes */

/* Host-visible outputs of one frame; valid until cairo_ctx_release(ticket). */
typedef struct cairo_frame_result {
  const uint8_t *block_table; /* wmb*hmb evx_block_desc (16 B, pack(2) layout) */
  const int16_t *coef_y;      /* output_cache Y, wa x ha, pitch wa (NULL      */
  const int16_t *coef_u;      /*   without CAIRO_OUT_COEF: cairo_ctx_fetch_coef) */
  const int16_t *coef_v;      /* output_cache V                               */
  uint32_t wa, ha, wmb, hmb;
  uint32_t index, type, quality;
  const uint32_t *feed;       /* CAIRO_OUT_FEED: feed bits, LSB-first words   */
  uint64_t feed_bits;
  int32_t feed_status;        /* CAIRO_FEED_*                                 */
} cairo_frame_result;

/* Context = one encoder's device state: R ring slots, input and output_cache
 * planes, block table, inter-search records, staging.  width/height are the
 * nominal frame size (aligned up to 16 internally, evx1enc.cpp:79-80); ring is
 * R = EVX_REFERENCE_FRAME_COUNT (1..4); device is the HIP ordinal. */
CAIRO_API int cairo_ctx_create(uint32_t width, uint32_t height, uint32_t ring, int device,
                               cairo_ctx **out);
/* The same with an explicit number of staging slots (frames in flight,
 * 2..256; cairo_ctx_create uses 96: three 32-frame launches, so that the
 * host entropy of one overlaps the GPU work of the next two).  A synchronous
 * caller (one frame in flight, as evx1_encoder::encode) needs 2: about
 * 0.35 GB of HBM for a 4K R = 4 context instead of 12 GB.  Frames per launch
 * are at most stages / 2. */
CAIRO_API int cairo_ctx_create_ex(uint32_t width, uint32_t height, uint32_t ring, int device,
                                  int stages, cairo_ctx **out);
CAIRO_API int cairo_ctx_destroy(cairo_ctx *ctx);
/* Zero every plane (fresh-encoder state, common.cpp:79-150) and clear a
 * reported in-kernel timeout, so the context is usable again. */
CAIRO_API int cairo_ctx_reset(cairo_ctx *ctx);

/* Submit frame (index, type 0=intra/1=inter, quality).  rgb is RGB888 with
 * pitch 3*width, in host memory (rgb_on_device = 0) or device memory of this
 * context's GPU (1; must stay valid until the frame's wait).  Frames are
 * encoded in batches of up to cairo_ctx_set_batch frames, pipelined on the GPU
 * in one launch; a batch launches when full or when a frame of it is waited
 * on.  Returns a ticket. */
CAIRO_API int cairo_ctx_submit(cairo_ctx *ctx, const uint8_t *rgb, int rgb_on_device,
                               uint32_t index, uint32_t type, uint32_t quality, int *ticket);
/* The same for a frame of any CAIRO_FMT_* with a row pitch (0: tight).  A host
 * frame is packed tight into the frame's staging slot on upload; a device
 * frame is read in place, at any byte alignment, and must lie inside one
 * allocation with all cairo_frame_layout bytes (else EVX_ERROR_INVALID_ARGS).
 * The frames of one launch may mix formats.  (RGB24, 0) is cairo_ctx_submit. */
CAIRO_API int cairo_ctx_submit_fmt(cairo_ctx *ctx, const uint8_t *frame, int on_device, int fmt,
                                   uint32_t pitch, uint32_t index, uint32_t type, uint32_t quality,
                                   int *ticket);

/* ---- scaled submit ---------------------------------------
 * One source frame in device memory feeds contexts of several sizes (the 4K
 * master and its 1080p and 720p renditions): each context reads it in place
 * and scales it to its own width x height on the GPU, before its convert.
 *
 * The rule is an area average in exact integers, applied to every 8-bit sample
 * plane as the format stores it: R, G and B of RGB24 / BGR24; Y8, U8 and V8 of
 * I420 / NV12, the chroma planes at half size in both axes.  Per axis, with S
 * samples of the source region and D output samples (chroma: both halved),
 * g = gcd(S, D), L = S / g, P = D / g: output sample o covers the units
 * [o L, (o + 1) L), source sample s the units [s P, (s + 1) P), and w(o, s) is
 * the length of their overlap (for one o the weights sum to L).  Then
 *   out(ox, oy) = (sum_sy sum_sx wy(oy, sy) wx(ox, sx) src(sx, sy)
 *                  + ((Lx Ly) >> 1)) / (Lx Ly)                  (floor division)
 * with no intermediate rounding.  S == D is a copy; an exact 2:1 is the mean
 * of a 2x2 block, halves rounded up.  The result is a tight frame of the same
 * format at the context's size, and everything downstream is what a tight
 * frame of that format gets: a scaled submit produces exactly the bits of
 * submitting the scaled frame.
 *
 * Constraints (EVX_ERROR_INVALID_ARGS): source width, height and the four crop
 * values even; the crop inside the source; D <= S <= 8 D on each axis
 * (downscale or copy, at most 8:1); 255 Lx Ly < 2^31; a source of at most
 * 32768 x 32768; reserved words 0.  The source must be device memory of the
 * context's GPU: the staging slot it is scaled into holds a frame of the
 * context's size, not a larger source, and uploading once and reading in place
 * is the point, so a host source is refused. */
typedef struct cairo_source {
  uint32_t width, height;                  /* size of the source frame (even)               */
  uint32_t crop_x, crop_y, crop_w, crop_h; /* region to scale; crop_w == 0 (then all four   */
                                           /* are 0): the whole frame                       */
  uint32_t reserved[2];                    /* 0                                             */
} cairo_source;
/* sizeof(cairo_source), for bindings. */
CAIRO_API int cairo_source_size(void);
/* Validity of scaling src (format fmt, row pitch `pitch` of the source, 0:
 * tight) to dst_w x dst_h; no device needed. */
CAIRO_API int cairo_scale_check(int fmt, uint32_t pitch, const cairo_source *src, uint32_t dst_w,
                                uint32_t dst_h);
/* cairo_ctx_submit_fmt of the frame that scaling src to the context's size
 * gives.  frame is device memory of this context's GPU, inside one allocation
 * with all cairo_frame_layout(fmt, src->width, src->height, pitch) bytes, at
 * any byte alignment; it is read when the frame's batch launches and must stay
 * valid until the frame's wait.  A launch may mix scaled and unscaled frames,
 * source sizes, crops and formats.  A refused submit takes no ticket. */
CAIRO_API int cairo_ctx_submit_scaled(cairo_ctx *ctx, const uint8_t *frame, int fmt, uint32_t pitch,
                                      const cairo_source *src, uint32_t index, uint32_t type,
                                      uint32_t quality, int *ticket);
/* Known-answer check of the scaling kernel on host buffers, without a context
 * or the engine.  out holds the tight dst_w x dst_h frame followed by
 * CAIRO_KAT_SCALE_GUARD more bytes; all of it is uploaded first, so bytes the
 * kernel must not touch (the guard) can be checked.  The device copy of frame
 * keeps frame's address modulo 4, so a misaligned source can be checked. */
#define CAIRO_KAT_SCALE_GUARD 64
CAIRO_API int cairo_kat_scale(int fmt, uint32_t pitch, const cairo_source *src, const uint8_t *frame,
                              uint32_t dst_w, uint32_t dst_h, uint8_t *out, int device);

/* ---- tensor frames -----------------------------------------
 * A frame that already lives in device memory as a tensor -- a model's output,
 * a loader's input -- is taken and written in place: planar or channels-last,
 * uint8 / float16 / bfloat16 / float32, values in any affine range, with any
 * positive strides (a frame of an NCHW batch, a channels_last view, a crop, the
 * RGB channels of an RGBA tensor). */
#define CAIRO_DT_U8   0
#define CAIRO_DT_F16  1   /* IEEE binary16 */
#define CAIRO_DT_BF16 2
#define CAIRO_DT_F32  3
typedef struct cairo_tensor {
  uint32_t dtype;        /* CAIRO_DT_*                                            */
  uint32_t reserved0;    /* 0                                                     */
  int64_t  stride[3];    /* in elements: channel (R,G,B = 0,1,2), row, column; >0 */
  float    mul[3], add[3];  /* per channel, finite                                */
  uint32_t reserved[2];  /* 0                                                     */
} cairo_tensor;
/* Element (c, y, x) is at base + (c*stride[0] + y*stride[1] + x*stride[2]) *
 * elem_size; the width W and height H are the context's.
 *
 * The map, in IEEE binary32, one stated rounding per step, nothing else:
 *   in  (dir 0), tensor element to 8-bit sample s:
 *     x = (float)element                      (exact for all four dtypes,
 *                                              float16 subnormals included)
 *     t = fmaf(x, mul[c], add[c])
 *     s = isnan(t) ? 0 : (int)min(max(rintf(t), 0.f), 255.f)
 *                                             (nearest, ties to even; +-inf clamp)
 *   out (dir 1), sample s to tensor element:
 *     t = fmaf((float)s, mul[c], add[c])
 *     F32: t.  F16 / BF16: t rounded to nearest even, overflow to infinity,
 *     subnormals kept.  U8: the clamp and round of dir 0.
 * For values in [0, 1]: in mul = 255, add = 0; out mul = 1/255, add = 0.
 *
 * Everything else is what a tight RGB24 frame gets: a tensor submit produces
 * exactly the bits of submitting pack(tensor) as RGB24, and a frame decoded
 * into a tensor is unpack of the RGB24 frame cairo_ctx_decode_frame writes.
 *
 * Validity (EVX_ERROR_INVALID_ARGS otherwise): a known dtype, reserved words
 * 0, finite mul and add, base aligned to the element size, 1 <= H <= 65535,
 * and no two elements at one address: the (stride, extent) pairs with extents
 * (3, H, W), sorted ascending by stride (ties by extent) into (s1,e1), (s2,e2),
 * (s3,e3), satisfy s1 >= 1, s2 >= s1*e1 and s3 >= s2*e2.  The span
 * 1 + sum (e_i - 1) * s_i is at most 2^40 elements.  Negative strides, BGR
 * order, host tensors and integer dtypes other than uint8 are not taken. */
/* sizeof(cairo_tensor), for bindings. */
CAIRO_API int cairo_tensor_size(void);
/* Validity of desc for a width x height frame at address base (only its
 * alignment is looked at); *span_bytes (may be NULL) receives the span in
 * bytes.  Host only, no device needed. */
CAIRO_API int cairo_tensor_check(const cairo_tensor *desc, const void *base, uint32_t width, uint32_t height,
                                 uint64_t *span_bytes);
/* The map as plain host loops, on host buffers: dir 0 reads tensor and writes
 * the tight RGB24 frame rgb24 (3*w*h bytes), dir 1 the reverse, writing only
 * the elements the descriptor covers.  The same per-sample code as the
 * kernels.  No device needed. */
CAIRO_API int cairo_tensor_host(int dir, const cairo_tensor *desc, uint32_t w, uint32_t h, void *tensor,
                                uint8_t *rgb24);
/* Known-answer check of the tensor kernels on host buffers, without a context
 * or the engine.  tensor is tensor_bytes long from element (0,0,0) (at least
 * the span); rgb24 holds the tight frame followed by CAIRO_KAT_TENSOR_GUARD
 * bytes.  Both are uploaded first and both are read back, so the bytes a
 * kernel must not touch can be checked.  The device copy of tensor keeps
 * tensor's address modulo 16, so a misaligned base can be checked. */
#define CAIRO_KAT_TENSOR_GUARD 64
CAIRO_API int cairo_kat_tensor(int dir, const cairo_tensor *desc, uint32_t w, uint32_t h, void *tensor,
                               uint64_t tensor_bytes, uint8_t *rgb24, int device);
/* cairo_ctx_submit of the RGB24 frame the input map gives.  base is device
 * memory of this context's GPU; the whole span lies inside one allocation (a
 * framework's sub-allocated block passes).  It is read when the frame's batch
 * launches, by one pre-pass kernel per launch that fills the frames' staging
 * slots, and must stay valid and unchanged until the frame's wait; the caller
 * orders its producer before the submit, as for any device frame.  A host
 * pointer is refused: the 3*W*H staging slot cannot stage a float frame.  A
 * launch may mix tensor frames of any dtype, strides and map with frames of
 * the pixel formats.  A refused submit takes no ticket.  Allowed for group
 * members. */
CAIRO_API int cairo_ctx_submit_tensor(cairo_ctx *ctx, const void *base, const cairo_tensor *desc, uint32_t index,
                                      uint32_t type, uint32_t quality, int *ticket);

/* ---- scaled tensor submit ----------------------------------
 * One tensor in device memory -- a model's 4K output, a frame of a loader's
 * batch -- feeds contexts of several sizes, with no packed full-size copy.  The
 * tensor has src->width x src->height elements per channel and is described by
 * a cairo_tensor exactly as for cairo_ctx_submit_tensor, with the source's
 * width and height in place of the context's; src is the scaled submit's
 * cairo_source (the source size and an optional even crop).
 *
 * Write pack for the input map of cairo_tensor (one fmaf, one rintf, a clamp,
 * NaN -> 0) and scale for the area average of the scaled submit on a tight
 * RGB24 frame.  The frame that is encoded is
 *     scale(pack(tensor))   to the context's width x height:
 * every source element is first mapped to its 8-bit sample, and the samples
 * are then averaged in exact integers,
 *     (sum wy wx s + ((Lx Ly) >> 1)) / (Lx Ly)                 (floor division)
 * with no intermediate rounding.  So a scaled tensor submit produces exactly
 * the bits of cairo_ctx_submit_scaled on the RGB24 frame pack(tensor), hence
 * those of cairo_ctx_submit of the scaled frame: a ladder fed from a tensor
 * gives the streams of a ladder fed from its packed copy.  (Rounding first,
 * then averaging, composes two maps that are specified already and keeps the
 * sum independent of its order; an average of floats would be neither.)
 *
 * Validity (EVX_ERROR_INVALID_ARGS; a refused submit takes no ticket):
 * cairo_tensor_check(desc, base, src->width, src->height) holds, and so does
 * every rule of cairo_scale_check(CAIRO_FMT_RGB24, 0, src, dst_w, dst_h): even
 * sizes and crop values, the crop inside the source, D <= S <= 8 D per axis,
 * 255 Lx Ly < 2^31, sides of at most 32768, reserved words 0.  The whole span
 * of the source lies inside one device allocation of the context's GPU; a host
 * pointer is refused.  Elements outside the crop are never read, the tensor is
 * never written, and nothing but the slot's tight 3*W*H frame is written. */
/* Validity of scaling the tensor (desc at address base, of which only the
 * alignment is looked at) of src's size to dst_w x dst_h; *span_bytes (may be
 * NULL) receives the span of the source tensor in bytes.  Host only, no device
 * needed. */
CAIRO_API int cairo_tensor_scale_check(const cairo_tensor *desc, const void *base, const cairo_source *src,
                                       uint32_t dst_w, uint32_t dst_h, uint64_t *span_bytes);
/* cairo_ctx_submit of the RGB24 frame scale(pack(tensor)) at the context's
 * size.  base, its lifetime and its ordering are cairo_ctx_submit_tensor's; it
 * is read when the frame's batch launches, by one pre-pass kernel per launch.
 * A launch may mix scaled tensor frames of any dtype, strides, map, source
 * size and crop with tensor, scaled and plain frames.  Allowed for group
 * members.  The drop-in encoder does not take them. */
CAIRO_API int cairo_ctx_submit_tensor_scaled(cairo_ctx *ctx, const void *base, const cairo_tensor *desc,
                                             const cairo_source *src, uint32_t index, uint32_t type,
                                             uint32_t quality, int *ticket);
/* Known-answer check of the kernel on host buffers, without a context or the
 * engine, with cairo_kat_tensor's conventions: tensor is tensor_bytes long
 * from element (0,0,0) (at least the span); rgb24 holds the tight dst_w x
 * dst_h frame followed by CAIRO_KAT_TENSOR_GUARD bytes.  Both are uploaded
 * first and both are read back.  The device copy of tensor keeps tensor's
 * address modulo 16. */
CAIRO_API int cairo_kat_tensor_scale(const cairo_tensor *desc, const cairo_source *src, void *tensor,
                                     uint64_t tensor_bytes, uint32_t dst_w, uint32_t dst_h, uint8_t *rgb24,
                                     int device);

/* Wait until the frame's block table and coefficients are host-visible. */
CAIRO_API int cairo_ctx_wait(cairo_ctx *ctx, int ticket, cairo_frame_result *out);
/* The decoder's hot path (decode_slice + deblock + convert_image,
 * decode.cpp:146-198): reconstruct frame `index` from its block table
 * (wmb*hmb 16-B descs) and coefficient planes (y | u | v contiguous, the
 * decoder's input_cache) into ring slot index % R, deblock it, and write it as
 * RGB888 (width*height*3, pitch 3*width) to host memory rgb.  Synchronous.
 * The engine trusts the descs: the caller checks them with cairo_table_check
 * first (the drop-in decoder does), and must not pass a table it refuses. */
CAIRO_API int cairo_ctx_decode_frame(cairo_ctx *ctx, const uint8_t *block_table, const int16_t *coef,
                                     uint32_t index, uint8_t *rgb);
/* The same, written as a frame of format fmt with row pitch `pitch` (0: tight)
 * to host memory out (cairo_frame_layout bytes; the pitch padding keeps its
 * bytes). */
CAIRO_API int cairo_ctx_decode_frame_fmt(cairo_ctx *ctx, const uint8_t *block_table, const int16_t *coef,
                                         uint32_t index, int fmt, uint32_t pitch, uint8_t *out);
/* The same, written into a tensor in device memory of this context's GPU (the
 * output map of cairo_tensor; base and desc as for cairo_ctx_submit_tensor):
 * unpack of the RGB888 frame cairo_ctx_decode_frame writes.  No copy to the
 * host is made.  Bytes of the destination that no element covers (stride
 * gaps, an alpha channel, everything beyond the span) are never written.
 * Synchronous, and refused for group members, like cairo_ctx_decode_frame. */
CAIRO_API int cairo_ctx_decode_frame_tensor(cairo_ctx *ctx, const uint8_t *block_table, const int16_t *coef,
                                            uint32_t index, void *base, const cairo_tensor *desc);
/* Hand the ticket's staging buffers back (required before ticket+stages). */
CAIRO_API int cairo_ctx_release(cairo_ctx *ctx, int ticket);
/* Launch any pending frames and block until all GPU work is finished. */
CAIRO_API int cairo_ctx_sync(cairo_ctx *ctx);
/* Staging slots = frames that may be in flight (submitted, not released). */
CAIRO_API int cairo_ctx_stages(const cairo_ctx *ctx);
/* Frames per engine launch, 1..min(32, stages/2) (default 32 for frames of up to
 * 16000 macroblocks, 28 above). */
CAIRO_API int cairo_ctx_set_batch(cairo_ctx *ctx, int frames);
/* The default frames per launch for a frame size (no device needed; 0 for an
 * empty size). */
CAIRO_API int cairo_default_batch(uint32_t width, uint32_t height);
/* The engine's (frame, row) task order for a launch of `frames` frames of hmb
 * macroblock rows: frames * hmb words (frame << 16 | row), sorted by row +
 * slope * frame; *slope receives the slope.  A launch's workers also take the
 * previous launch's tasks, merged by the same key with that launch's frames
 * first (no device needed; for tests of the deadlock-freedom argument). */
CAIRO_API int cairo_task_order(int hmb, int frames, int32_t *out, int *slope);
/* The queues of one pool (0 row helpers, 1 row coders) of a launch of one
 * context with n_helpers + n_rows workers (kernels.h kLabels): the same tasks
 * as cairo_task_order, stably partitioned by label, label l's queue being
 * order[seg[l] .. seg[l+1]) (seg: 9 words).  *nlab receives 8 where the engine
 * bands that pool (frames of at least 100 macroblock rows, both worker counts
 * multiples of 8: one queue per XCD), else 1 (seg = {0, total, ...}) -- the
 * predicate the launch itself applies.  No device needed. */
CAIRO_API int cairo_task_queues(int hmb, int frames, int n_helpers, int n_rows, int pool, int32_t *order,
                                int32_t *seg, int *nlab);

/* Introspection (synchronous; of the last submitted frame).  which: 0 input,
 * 1 output_cache, 2+k ring slot k. */
CAIRO_API int cairo_ctx_read_planes(cairo_ctx *ctx, int which, int16_t *y, int16_t *u,
                                    int16_t *v);
/* Inter-search records of the last frame: (ring-1)*mbs descs and SADs. */
CAIRO_API int cairo_ctx_read_inter(cairo_ctx *ctx, uint8_t *descs, int32_t *sads);
CAIRO_API int cairo_ctx_read_table(cairo_ctx *ctx, uint8_t *table);
/* Debug: flags & 1 snapshots the reconstruction before the deblock of every
 * frame (cairo_ctx_read_predeblock returns the last snapshot); flags & 2
 * records per-macroblock phase timestamps of the wavefront kernel (12 x u64
 * per MB, 100 MHz clock; cairo_ctx_read_stamps). */
CAIRO_API int cairo_ctx_set_debug(cairo_ctx *ctx, int flags);
CAIRO_API int cairo_ctx_read_stamps(cairo_ctx *ctx, uint64_t *out);
/* Which instantiation of the engine the last launch enqueued by this context
 * runs (no synchronization; 0 before the first launch): 0 the plain one (no
 * diagnostics compiled in, agent-scope hand-offs only), 1 the general one --
 * chosen for a launch with stamps, trace or the inject flag set, one whose
 * frames (or those of the previous launch it shares queues with) belong to a
 * group across devices or processes, and every decode launch. */
CAIRO_API int cairo_ctx_engine_variant(cairo_ctx *ctx);
/* Debug: flags & 4 keeps a live per-workgroup state trace of the engine in
 * mapped host memory; read it (n int32 words) without synchronizing.
 * flags & 8 (test hook) marks the device's sticky timeout word as if an
 * in-kernel wait had timed out: every later frame reports
 * EVX_ERROR_HARDWAREFAIL until cairo_ctx_reset. */
CAIRO_API int cairo_ctx_read_trace(cairo_ctx *ctx, int32_t *out, int n);
/* flags & 16 (test hook) makes the row helpers of MB row min(1, hmb-1) of
 * every frame launched from now on record a timeout of their first progress
 * wait through the device's own reporting path (CAIRO_WAIT_INJECTED), without
 * waiting; setting flags without 16 clears it. */

/* The in-kernel wait that timed out first, as the last frame that reported
 * EVX_ERROR_HARDWAREFAIL saw it (zeros: none since create / reset).  Up to 16
 * int32 words: kind (CAIRO_WAIT_*), the waiting frame's epoch, its stream
 * index, its MB row, the group member (0 alone), what it needed (columns, a
 * count or a tag), what it waited on (CAIRO_WAIT_RECORDS: inter group;
 * _GRANULE: macroblock index; _PREV_PROGRESS / _INJECTED: row | back << 16;
 * _ROW_ABOVE: row), and the last value it saw (low, high word). */
#define CAIRO_WAIT_RECORDS 1
#define CAIRO_WAIT_GRANULE 2
#define CAIRO_WAIT_PREV_PROGRESS 3
#define CAIRO_WAIT_ROW_ABOVE 4
#define CAIRO_WAIT_BATCH 5
#define CAIRO_WAIT_INJECTED 6
#define CAIRO_WAIT_HOST_MARK 9
CAIRO_API int cairo_ctx_timeout_info(cairo_ctx *ctx, int32_t *out, int n);
/* Debug: flags & 32 turns on the engine's time accounting, which a library
 * built with CAIRO_ACCT=1 (tools/build_variant.sh) fills: per role and phase,
 * the 10 ns ticks summed over every task since the last reset, then bytes
 * requested by the window staging and the polls (24 words, kernels.h Acct;
 * zeros from a regular build).  Synchronous; reset = 1 zeroes
 * the counters after reading them. */
CAIRO_API int cairo_ctx_read_acct(cairo_ctx *ctx, uint64_t *out, int n, int reset);
CAIRO_API int cairo_ctx_read_predeblock(cairo_ctx *ctx, int16_t *y, int16_t *u, int16_t *v);

/* Per-kernel timing (HIP events on the kernels' stream), opt-in. */
CAIRO_API int cairo_ctx_set_profiling(cairo_ctx *ctx, int enable);
/* Accumulated ms per kernel since the last call: [convert, 0 (inter search
 * runs inside the engine), engine (inter search + row coding + in-loop
 * deblock) summed over launches, engine busy time = the length of the union
 * of the launches' intervals (two launches run at once, so the sum counts
 * overlapped time twice)], and the number of frames they cover; resets the
 * accumulators.  Enabling profiling starts the common clock of the busy
 * intervals. */
CAIRO_API int cairo_ctx_take_timings(cairo_ctx *ctx, double ms[4], int *frames);
/* The engine launches' [start, end) intervals (ms on the profiling clock,
 * pairs, sorted by start) collected since the last cairo_ctx_take_timings,
 * without resetting them: the busy-time union can be recomputed from them.
 * *n receives the count; at most cap pairs are written. */
CAIRO_API int cairo_ctx_busy_intervals(cairo_ctx *ctx, double *out, int cap, int *n);
/* Row-coder workgroups of the engine per launch (0 = automatic: a quarter of
 * the device's resident engine workgroups, 192 on a full MI355X; larger
 * values are rejected, since every launch must stay co-resident with the
 * one before it). */
CAIRO_API int cairo_ctx_set_workgroups(cairo_ctx *ctx, int mb_rows);

/* ---- frame-interleaved groups (multi-GPU single stream) ----
 * N contexts (one per GPU and process, or several on one device) encode ONE
 * stream: member k encodes the frames n = k (mod N), in order, reading the
 * other members' reconstructions (references, the stale rows of frame n-R),
 * output_cache (copy macroblocks) and deblock progress in place -- over xGMI
 * when they live on other GPUs.  The hand-off is a per-row progress word; no
 * collective and no copy is on the data path.  Output is the single-context
 * stream, bit for bit.
 *
 * Protocol: create every member (same width, height, ring), call
 * cairo_ctx_peer_info on each (cross_device = 1 if any member is another
 * process or device: the shared buffers are then re-allocated fine-grained),
 * exchange the records (any transport: they are plain bytes), then
 * cairo_ctx_join_group on each with all N records in rank order, before any
 * frame.  Submit frame n to member n % N with index n; before waiting on a
 * frame, every member must have launched (cairo_ctx_flush) its frames that
 * precede it in the stream -- a member's in-kernel wait on another's
 * unlaunched frame times out after 2 s (EVX_ERROR_HARDWAREFAIL).  Members on
 * one device share its workgroup slots: give each cairo_ctx_max_workgroups /
 * (members on the device) row coders (cairo_ctx_set_workgroups).
 * cairo_ctx_reset leaves the group. */
#define CAIRO_MAX_COEF_CHUNKS 16
typedef struct cairo_peer {
  uint32_t width, height, ring;
  int32_t device, pid, stages, fine_grained;
  int32_t coef_chunks;      /* the output_cache slots live in this many allocations */
  int32_t coef_chunk_slots; /* staging slots per chunk: slot s is in chunk s / coef_chunk_slots */
  int32_t reserved;
  uint64_t ring_addr, progress_addr;             /* device addresses in the owner's process */
  uint64_t coef_addr[CAIRO_MAX_COEF_CHUNKS];
  uint8_t ipc_ring[64], ipc_progress[64];        /* hipIpcMemHandle_t of each allocation */
  uint8_t ipc_coef[CAIRO_MAX_COEF_CHUNKS][64];
} cairo_peer;
/* A member's output_cache (2 bytes x 1.5 x Wa x Ha per staging slot) is
 * allocated in chunks of at most 1 GiB, each exported with its own IPC handle:
 * an IPC import of a single fine-grained allocation of 2 GiB or more never
 * returned on the test boxes (a 4K member with 96 slots has 2.4 GB of it). */
/* sizeof(cairo_peer), for bindings that exchange the records as bytes. */
CAIRO_API int cairo_peer_size(void);
CAIRO_API int cairo_ctx_peer_info(cairo_ctx *ctx, int cross_device, cairo_peer *out);
CAIRO_API int cairo_ctx_join_group(cairo_ctx *ctx, int size, int rank, const cairo_peer *peers);
/* Whether local_members group members may share one process and device:
 * they need GPU_MAX_HW_QUEUES >= 3 * local_members + 2 (at most 32), or two
 * members' persistent launches can land in one in-order hardware queue and
 * deadlock.  hw_queues < 0: the process's GPU_MAX_HW_QUEUES as read when the
 * library was loaded (the HIP runtime reads it once, when it starts: set it
 * before the process starts; 4 when unset).  0 = fine (always for fewer than
 * 2), else EVX_ERROR_INVALID_ARGS with a message on stderr.
 * cairo_ctx_join_group applies it with hw_queues = -1; no device needed. */
CAIRO_API int cairo_group_check_queues(int local_members, int hw_queues);
/* Launch the pending (partial) batch now. */
CAIRO_API int cairo_ctx_flush(cairo_ctx *ctx);
/* Choose the outputs (CAIRO_OUT_COEF and/or CAIRO_OUT_FEED) for frames
 * submitted from now on; no frame may be in flight. */
CAIRO_API int cairo_ctx_set_outputs(cairo_ctx *ctx, int outputs);
/* The coefficient planes of a waited, unreleased frame (a D2H copy from its
 * staging slot when the context does not copy them already). */
CAIRO_API int cairo_ctx_fetch_coef(cairo_ctx *ctx, int ticket, cairo_frame_result *out);
/* Of a launch's 2 * workgroups workers, how many are row helpers (inter
 * search + deblock) rather than row coders (0: half). */
CAIRO_API int cairo_ctx_set_helpers(cairo_ctx *ctx, int helpers);
/* Upper bound of cairo_ctx_set_workgroups on this device. */
CAIRO_API int cairo_ctx_max_workgroups(const cairo_ctx *ctx);

/* ---- per-frame distortion and kept reconstructions --------
 * A frame's deblocked reconstruction lives in ring slot index % R and is
 * overwritten R frames later, inside the same launch.  With any of the flags
 * below the deblock also stores it into a plane set of the frame's staging
 * slot (the "keep"), which stays valid until the ticket is released; the
 * metric flags run a reduction kernel over it after the launch. */
#define CAIRO_METRIC_SSE 1  /* exact sum of squared errors per plane          */
#define CAIRO_METRIC_SSIM 2 /* sum of SSIM window values per plane            */
#define CAIRO_KEEP_RECON 4  /* keep the reconstruction (implied by a metric)  */
/* Both sides are compared as the 8-bit samples the I420 output defines,
 * Y8 = clamp(Y - 16, 0, 255), U8 = clamp(U, 0, 255), V8 = clamp(V, 0, 255),
 * over the nominal picture: width x height luma, (width/2) x (height/2)
 * chroma (index 0 Y, 1 U, 2 V); the padding up to 16 is excluded.  a is the
 * source (what an I420 submit carried, or the converted RGB), b the
 * reconstruction (what the decoder shows as I420).  Under an input colour
 * description a is the source after the map: what a full-range BT.601 I420
 * submit of the mapped frame would carry.
 *   sse[p]      sum of (a - b)^2, exact.  PSNR = 10 log10(255^2 * samples[p] /
 *               sse[p]), infinite at sse 0; "all planes" uses the summed sse
 *               over the summed samples.
 *   SSIM        the plane is cut into 4x4 blocks from its origin, bw =
 *               floor(pw/4) by bh = floor(ph/4); leftover columns and rows are
 *               ignored.  A window is 2x2 blocks (8x8 samples) at block stride
 *               1: (bw-1)*(bh-1) windows, none if bw < 2 or bh < 2.  Over a
 *               window's 64 samples, in integers: s1 = sum a, s2 = sum b,
 *               ss = sum (a^2 + b^2), s12 = sum a*b;
 *                 vars  = 64*ss - s1^2 - s2^2,  covar = 64*s12 - s1*s2,
 *                 c1 = 416, c2 = 235963   ((0.01*255)^2*64, (0.03*255)^2*64*63)
 *                 num = (2*s1*s2 + c1) * (2*covar + c2)
 *                 den = (s1^2 + s2^2 + c1) * (vars + c2)        (exact in int64)
 *               and the window's value is (double)num / (double)den.
 *   ssim_sum[p] the sum of the plane's window values (a fixed reduction order:
 *               the same input gives the same bits), ssim_windows[p] their
 *               count; SSIM = ssim_sum / ssim_windows.
 * Fields of a metric that was not asked for are 0. */
typedef struct cairo_frame_metrics {
  uint32_t flags;          /* the CAIRO_METRIC_* computed for this frame */
  uint32_t width, height;  /* nominal frame size */
  uint32_t reserved;
  uint64_t sse[3];
  double ssim_sum[3];
  uint64_t ssim_windows[3];
  uint64_t samples[3];
} cairo_frame_metrics;
/* sizeof(cairo_frame_metrics), for bindings. */
CAIRO_API int cairo_frame_metrics_size(void);
/* Choose the flags for frames submitted from now on; no frame may be in
 * flight (EVX_ERROR_INVALID_RESOURCE).  The first enabling call allocates
 * `stages` plane sets (3 * Wa * Ha bytes each: 2.4 GB for a 4K context with 96
 * stages; EVX_ERROR_OUTOFMEMORY leaves the context as it was), flags 0 frees
 * them; with flags 0 a launch is what it is without this call.  Survives
 * cairo_ctx_reset.  EVX_ERROR_INVALID_ARGS for unknown bits and for a member
 * of a group (whose deblock already pushes to its mirrors); a context with
 * metrics on cannot join a group. */
CAIRO_API int cairo_ctx_set_metrics(cairo_ctx *ctx, int flags);
/* The metrics of a waited, unreleased frame.  EVX_ERROR_INVALID_ARGS when no
 * metric was on for it, for a decoded frame, and for a ticket that is not
 * waited or already released. */
CAIRO_API int cairo_ctx_frame_metrics(cairo_ctx *ctx, int ticket, cairo_frame_metrics *out);
/* The kept reconstruction of a waited, unreleased frame as aligned int16
 * planes, in the layout of cairo_ctx_read_planes (Wa x Ha, Wa/2 x Ha/2); any
 * of y, u, v may be NULL.  Refused like cairo_ctx_frame_metrics. */
CAIRO_API int cairo_ctx_fetch_recon_planes(cairo_ctx *ctx, int ticket, int16_t *y, int16_t *u, int16_t *v);
/* The same frame in any CAIRO_FMT_* with row pitch `pitch` (0: tight) into
 * host memory out (cairo_frame_layout bytes; the pitch padding keeps its
 * bytes): what cairo_ctx_decode_frame_fmt writes for this frame. */
CAIRO_API int cairo_ctx_fetch_recon(cairo_ctx *ctx, int ticket, int fmt, uint32_t pitch, uint8_t *out);
/* The same frame as RGB888 through the output map into a tensor in device
 * memory (cairo_ctx_decode_frame_tensor's rules): what
 * cairo_ctx_decode_frame_tensor writes for this frame. */
CAIRO_API int cairo_ctx_fetch_recon_tensor(cairo_ctx *ctx, int ticket, void *base, const cairo_tensor *desc);
/* Known-answer check of the metrics kernels on host buffers, without a
 * context or the engine: planes a and b of w x h (luma; chroma (w/2) x (h/2))
 * with pitch_elems elements per luma row and pitch_elems / 2 per chroma row
 * (pitch_elems even, >= w), both metrics. */
CAIRO_API int cairo_kat_metrics(uint32_t w, uint32_t h, uint32_t pitch_elems, const int16_t *a_y,
                                const int16_t *a_u, const int16_t *a_v, const int16_t *b_y,
                                const int16_t *b_u, const int16_t *b_v, cairo_frame_metrics *out,
                                int device);

/* ---- target bitrate ---------------------------------------
 * With a cairo_rate set, the context chooses one quality per launch on the
 * device, from the sizes of the frames of earlier launches; the host is not in
 * the loop.  A frame's size is known on the device from its feed alone: the
 * arithmetic coder's adaptive model keeps plain counts, so its output for a
 * feed of N bits with z zeros is log2((N+1)! / (z! (N-z)!)) bits within its
 * termination, whatever their order.  The integer estimate of that is
 *
 *   L(x), 1 <= x < 2^32, Q16:  e = 31 - clz(x);  y = x << (31 - e);  sixteen
 *     times: y = (y * y) >> 31 (64-bit product), append bit (y >= 2^32), and if
 *     that bit is set y >>= 1;  L = (e << 16) | the sixteen bits
 *   E(N, z) = (N L(N) - z L(z) - (N-z) L(N-z)) >> 16   (a term with a zero
 *     factor is 0; N < 2^32, z <= N)
 *
 * and a frame counts as E + 80 bits (its 10-byte frame record; the stream
 * header is not counted), or 4 * target_bits when its feed overflowed.
 *
 * The control law is a pure function on cairo_rate_state.  P is the last
 * launch, O the one before, each {n frames, quality q, aim}; T = target_bits,
 * W = window.  step(n_new, obs_sum), obs_sum the summed bits of O's frames:
 *   fewer than two launches so far:  q = q0, aim = T
 *   otherwise:
 *     debt += obs_sum - O.n T                        (kept within +-2^60)
 *     Dp  = debt + P.n (P.aim - T)
 *     aim = clamp(T - Dp / W, max(T / 4, 1), 4 T)    (division toward zero)
 *     M = obs_sum / O.n;  s = max(0, bitlen(max(M, aim)) - 24)
 *     m = M >> s;  t = max(aim >> s, 1)
 *     qm = (O.q m^2 + t^2 / 2) / t^2                 (uint64)
 *     st = 1 + P.q / 4
 *     q = clamp(qm, P.q - st, P.q + st)
 *   q = clamp(q, qmin, qmax);  O = P;  P = {n_new, q, aim} */
typedef struct cairo_rate {
  uint32_t target_bits;  /* T, per frame: 1 .. 2^28 */
  uint32_t q0;           /* the quality of the first two launches, 1..31 */
  uint32_t qmin, qmax;   /* 1 <= qmin <= qmax <= 31 */
  uint32_t window;       /* W >= 1: frames over which a debt is paid back */
  uint32_t reserved[3];  /* 0 */
} cairo_rate;
typedef struct cairo_rate_state {
  int64_t debt;          /* observed bits minus T per observed frame */
  int64_t p_aim, o_aim;
  int32_t p_n, p_q, o_n, o_q;
  uint32_t launches;
  uint32_t reserved;
} cairo_rate_state;
typedef struct cairo_rate_info {
  uint32_t quality;      /* the quality the frame was coded with */
  uint32_t overflow;     /* its feed overflowed (feed_bits and ones are 0) */
  uint64_t feed_bits;    /* N */
  uint64_t ones;         /* set bits among them */
  int64_t est_bits;      /* E(N, N - ones) + 80; 4 T on overflow */
  int64_t aim;           /* bits per frame its launch aimed at */
  int64_t debt;          /* the state's debt after its launch's step */
} cairo_rate_info;
/* sizeof of the three, for bindings. */
CAIRO_API int cairo_rate_size(void);
CAIRO_API int cairo_rate_state_size(void);
CAIRO_API int cairo_rate_info_size(void);
/* Host only, no device needed.  E(N, zeros); -1 for N >= 2^32 or zeros > N. */
CAIRO_API int64_t cairo_rate_estimate(uint64_t nbits, uint64_t zeros);
/* A fresh state for cfg; EVX_ERROR_INVALID_ARGS for a bad configuration
 * (a field out of the ranges above, a reserved word set). */
CAIRO_API int cairo_rate_init(cairo_rate_state *state, const cairo_rate *cfg);
/* One step of the law: *q is the quality of the next launch's n_new frames
 * (1 .. 65535), obs_sum (0 .. 2^48) as above.  EVX_ERROR_INVALID_ARGS leaves
 * the state as it was. */
CAIRO_API int cairo_rate_step(cairo_rate_state *state, const cairo_rate *cfg, int n_new, int64_t obs_sum,
                              uint32_t *q);
/* Turn the controller on (a fresh state for cfg) or, with cfg NULL, off.
 * EVX_ERROR_INVALID_RESOURCE with a frame in flight (submitted and not
 * released); EVX_ERROR_INVALID_ARGS for a bad configuration, for a context
 * whose outputs do not include CAIRO_OUT_FEED, and for a member of a group.  A
 * refused call changes nothing.  While it is on: every launch is preceded by
 * one step, whose quality all its frames are coded with (the quality of a
 * submit is still validated, and otherwise unused); cairo_frame_result.quality
 * reports the chosen value; cairo_ctx_reset restarts the controller;
 * cairo_ctx_join_group (EVX_ERROR_INVALID_ARGS), cairo_ctx_set_outputs without
 * CAIRO_OUT_FEED (EVX_ERROR_INVALID_ARGS) and cairo_ctx_decode_frame*
 * (EVX_ERROR_INVALID_RESOURCE) are refused.  Launch L is stepped with the
 * frames of launch L-2, by stream order alone: for one sequence of calls
 * (submits, batch size, flushes, waits of unlaunched frames) the qualities are
 * always the same.  While it is off, a launch is what it is without this
 * call. */
CAIRO_API int cairo_ctx_set_rate(cairo_ctx *ctx, const cairo_rate *cfg);
/* What the controller saw and chose for a waited, unreleased frame that was
 * submitted while it was on; EVX_ERROR_INVALID_ARGS otherwise. */
CAIRO_API int cairo_ctx_frame_rate(cairo_ctx *ctx, int ticket, cairo_rate_info *info);
/* Known-answer check of the observing kernels on host buffers, without a
 * context or the engine: `total_words` words are uploaded whole, frame j's
 * feed is the nbits[j] bits from word base_words + j * stride_words on (it
 * must lie inside the buffer; count 1..48).  Bits beyond nbits[j] may be set:
 * they are not counted.  Out, per frame: feed_bits, ones and est_bits (the
 * other fields 0). */
CAIRO_API int cairo_kat_rate_observe(const uint32_t *words, uint64_t total_words, uint64_t base_words,
                                     uint64_t stride_words, const uint64_t *nbits, int count,
                                     cairo_rate_info *out, int device);

/* Known-answer check of the device transform chain: count macroblocks of 384
 * int16 (block-major: Y TL,TR,BL,BR, U, V; 64 each).  qtype[2m] = block type,
 * qtype[2m+1] = frame quality.  Host buffers in and out. */
CAIRO_API int cairo_kat_transform(const int16_t *src, const int16_t *pred, const uint8_t *qtype,
                                  int count, int16_t *coef, int16_t *recon, int32_t *qvar,
                                  int device);

/* Known-answer check of the device quantizer and dequantizer alone: count
 * (>= 1) macroblocks of 384 int16 coefficients in cairo_kat_transform's
 * layout.  tq[2m] = block type (0..3: a type with the copy bit has no
 * coefficients and is refused), tq[2m+1] = the quantizer parameter qp itself,
 * 1..31, not a quality.  Out: every element quantized, and that value
 * dequantized.  Host buffers in and out. */
CAIRO_API int cairo_kat_quant(const int16_t *coef, const uint8_t *tq, int count, int16_t *quant,
                              int16_t *dequant, int device);

/* Known-answer check of the GPU entropy precode (the kernels behind
 * CAIRO_OUT_FEED) on host buffers, without a context or the engine: count
 * frames (1..48, the most one launch holds) of wmb x hmb macroblocks (at most
 * 65535) and ring 1..4, frame j's block table at tables + j * wmb * hmb * 16
 * and its coefficient planes (pitch wmb * 16, chroma wmb * 8) at
 * coef_y + j * wmb * hmb * 256 and coef_u / coef_v + j * wmb * hmb * 64.  The
 * tables need not be legal: the precode reads what the serializer reads.
 * Frame j uses staging slot slot[j] of nslots (count <= nslots <= 48; the
 * slots distinct).  Every slot's device feed buffer, header and scratch, and
 * every frame's host buffer, hold the word `prefill` before the launch, which
 * is the one a context makes for a batch (precode, then the copy to the host
 * buffers).  Out, per frame: hdr[16] as copied (bits lo, hi; overflow flag;
 * dropped writes; the start bit of each of the 11 lists; one unused word);
 * the first feed_words words of its host buffer after the header, copied or
 * still `prefill`; and guard_words words of its slot's device feed buffer from
 * word (bits + 31) / 32 on -- from word 0 when the overflow flag is set -- with
 * `prefill` for words beyond the slot's end: one zeroed word (none on
 * overflow), then words no kernel may have touched. */
CAIRO_API int cairo_kat_precode(uint32_t wmb, uint32_t hmb, uint32_t ring, int count, int nslots,
                                const int32_t *slot, const uint8_t *tables, const int16_t *coef_y,
                                const int16_t *coef_u, const int16_t *coef_v, uint32_t prefill, uint32_t *hdr,
                                uint32_t *feed, uint64_t feed_words, uint32_t *guard, uint32_t guard_words,
                                int device);

/* Known-answer check of the pixel-format kernels on host buffers, without a
 * context or the engine.  dir 0: frame (fmt, pitch) -> tight int16 planes (w
 * and w/2 elements per row) through the input kernel.  dir 1: planes -> frame
 * through the output kernel; frame's previous contents are uploaded first, so
 * bytes the kernel must not touch can be checked. */
CAIRO_API int cairo_kat_convert(int dir, int fmt, uint32_t w, uint32_t h, uint32_t pitch, uint8_t *frame,
                                int16_t *y, int16_t *u, int16_t *v, int device);
/* The same under a colour description of the frame (dir 0: its input map,
 * dir 1: its output map; ignored for the RGB formats).  cairo_kat_convert is
 * (CAIRO_RANGE_FULL, CAIRO_MATRIX_BT601). */
CAIRO_API int cairo_kat_convert_color(int dir, int fmt, int range, int matrix, uint32_t w, uint32_t h,
                                      uint32_t pitch, uint8_t *frame, int16_t *y, int16_t *u, int16_t *v,
                                      int device);

/* ---- host entropy stage (serialize_slice, serialize.cpp:319-340) ---------
 * Appends the ABAC payload of one frame to out (LSB-first bit order) at bit
 * *bit_pos, advancing it.  coef planes have pitch wa (luma) / wa/2 (chroma). */
CAIRO_API int cairo_serialize_slice(const uint8_t *block_table, uint32_t wmb, uint32_t hmb,
                                    uint32_t ring, const int16_t *coef_y, const int16_t *coef_u,
                                    const int16_t *coef_v, uint8_t *out, uint32_t out_bytes,
                                    uint32_t *bit_pos);

/* The same payload from a frame's GPU-precoded feed (cairo_frame_result.feed
 * with CAIRO_FEED_VALID): only the arithmetic coder runs. */
CAIRO_API int cairo_serialize_feed(const uint32_t *feed, uint64_t feed_bits, uint8_t *out,
                                   uint32_t out_bytes, uint32_t *bit_pos);
/* The host precode alone (serialize.cpp:10-286, stream.cpp:550-581,
 * golomb.cpp:8-91, with the 32 Mbit per-section drop rule): the feed bits the
 * arithmetic coder consumes, LSB-first in 32-bit words -- what the GPU precode
 * writes for a CAIRO_FEED_VALID frame.  *feed_bits receives the bit count;
 * EVX_ERROR_CAPACITY_LIMIT (7) if feed_words cannot hold them. */
CAIRO_API int cairo_precode_slice(const uint8_t *block_table, uint32_t wmb, uint32_t hmb, uint32_t ring,
                                  const int16_t *coef_y, const int16_t *coef_u, const int16_t *coef_v,
                                  uint32_t *feed, uint64_t feed_words, uint64_t *feed_bits);

/* ---- host entropy decode (unserialize_slice, unserialize.cpp:321-342) ----
 * Decodes the ABAC payload of one frame starting at bit *read_index of data
 * (LSB-first, up to write_index) into the block table (wmb*hmb 16-B descs) and
 * the coefficient planes, which persist across frames: fields a block does not
 * carry keep their previous values, as in the reference decoder's context.
 * Advances *read_index.  EVX_ERROR_INVALID_RESOURCE (8) on a corrupt payload. */
CAIRO_API int cairo_unserialize_slice(const uint8_t *data, uint32_t *read_index, uint32_t write_index,
                                      uint32_t wmb, uint32_t hmb, uint32_t ring, uint8_t *block_table,
                                      int16_t *coef_y, int16_t *coef_u, int16_t *coef_v);

/* ---- legality of a decoded block table (host only, no device) -------------
 * 1 when the decode-mode engine reconstructs every desc of the table (wmb*hmb
 * 16-B descs) as the reference decoder does, else 0.  Every table the
 * reference encoder can write passes.  Per macroblock at (px, py):
 *   - block_type in {0, 1, 2, 3, 4, 6, 7} (decode.cpp:14-142);
 *   - without the copy bit: 1 <= q_index <= 31 (quantize.cpp:65-68);
 *   - without the intra bit: 1 <= prediction_target <= ring-1
 *     (encode.cpp:17-67);
 *   - with the motion bit: sp_pred <= 1, and when set sp_amount <= 1 and
 *     sp_index <= 7; the block at the vector and, when sp_pred, at its sub-pel
 *     neighbour (motion.cpp:61-109) lies inside the wmb*16 x hmb*16 frame;
 *   - intra with motion: both points (x, y) also lie in [px-32, px+32] x
 *     [py-48, py+16] and outside the region not yet coded,
 *     !(y > py-16 && x > px-16) (motion.cpp:238-241, 303-306).
 * A stream of ring size 3 that used target 2 arrives with target 0 (one target
 * bit, serialize.cpp:179) and is refused. */
CAIRO_API int cairo_table_check(const uint8_t *block_table, uint32_t wmb, uint32_t hmb, uint32_t ring);
/* The same rules desc by desc: ok[k] = 1 when descs[k] is legal as macroblock
 * mb_index[k] (raster index) of such a frame, else 0; a table is legal when
 * each of its descs is legal at its own index.  Returns 0, or
 * EVX_ERROR_INVALIDARG (1). */
CAIRO_API int cairo_desc_check(const uint8_t *descs, const uint32_t *mb_index, uint32_t n, uint32_t wmb,
                               uint32_t hmb, uint32_t ring, uint8_t *ok);

/* ---- frame pipeline ---------------------------------
 * GPU hot path + host entropy for a stream of frames: the caller submits
 * frames, a completion thread picks up each frame's outputs, a pool of entropy
 * workers runs serialize_slice on them in parallel (frames are
 * entropy-independent: the ABAC model restarts per slice, serialize.cpp:323),
 * and collect appends a frame's payload bits.  Appending the frame descriptors
 * and payloads in ticket order yields the reference stream (evx1enc.cpp:119-168).
 * The stream drives ctx exclusively while it exists (no direct cairo_ctx_submit
 * / wait / release); destroy it before the context.  A host RGB source must
 * stay valid until its frame is collected. */
typedef struct cairo_stream cairo_stream;
/* threads: entropy workers (0 = hardware threads - 1, at most 15). */
CAIRO_API int cairo_stream_create(cairo_ctx *ctx, int threads, cairo_stream **out);
/* Blocks while the frame's staging slot (ticket - stages) is still being
 * entropy-coded; EVX_ERROR_INVALID_RESOURCE (8) if ticket - 2*stages has not
 * been collected. */
CAIRO_API int cairo_stream_submit(cairo_stream *s, const uint8_t *rgb, int rgb_on_device,
                                  uint32_t index, uint32_t type, uint32_t quality, int *ticket);
/* cairo_stream_submit for a frame of any format (cairo_ctx_submit_fmt). */
CAIRO_API int cairo_stream_submit_fmt(cairo_stream *s, const uint8_t *frame, int on_device, int fmt,
                                      uint32_t pitch, uint32_t index, uint32_t type, uint32_t quality,
                                      int *ticket);
/* cairo_stream_submit for a scaled frame (cairo_ctx_submit_scaled). */
CAIRO_API int cairo_stream_submit_scaled(cairo_stream *s, const uint8_t *frame, int fmt, uint32_t pitch,
                                         const cairo_source *src, uint32_t index, uint32_t type,
                                         uint32_t quality, int *ticket);
/* cairo_stream_submit for a tensor frame (cairo_ctx_submit_tensor). */
CAIRO_API int cairo_stream_submit_tensor(cairo_stream *s, const void *base, const cairo_tensor *desc, uint32_t index,
                                         uint32_t type, uint32_t quality, int *ticket);
/* cairo_stream_submit for a scaled tensor frame (cairo_ctx_submit_tensor_scaled). */
CAIRO_API int cairo_stream_submit_tensor_scaled(cairo_stream *s, const void *base, const cairo_tensor *desc,
                                                const cairo_source *src, uint32_t index, uint32_t type,
                                                uint32_t quality, int *ticket);
/* Wait for the frame's payload and append it at bit *bit_pos of out
 * (out_bytes capacity, LSB-first; out == NULL only advances *bit_pos).  If it
 * does not fit, returns EVX_ERROR_CAPACITY_LIMIT (7) and keeps the payload:
 * collect again with a larger buffer. */
CAIRO_API int cairo_stream_collect(cairo_stream *s, int ticket, uint8_t *out, uint64_t out_bytes,
                                   uint64_t *bit_pos);
/* Wait for the frame's payload and return its size in bits (not collected). */
CAIRO_API int cairo_stream_payload_bits(cairo_stream *s, int ticket, uint64_t *nbits);
/* Diagnostic timeline of a collected frame (valid until ticket + 2*stages is
 * submitted): t[5] = submitted, outputs on the host, entropy start, entropy
 * end, collected; microseconds of a monotonic clock. */
CAIRO_API int cairo_stream_timeline(cairo_stream *s, int ticket, double *t);
/* The metrics of a frame of a context with cairo_ctx_set_metrics on (set
 * before the stream is created): copied when the pipeline picks up the
 * frame's outputs, valid for a collected frame until ticket + 2*stages is
 * submitted.  EVX_ERROR_INVALID_ARGS when the frame has none. */
CAIRO_API int cairo_stream_frame_metrics(cairo_stream *s, int ticket, cairo_frame_metrics *out);
/* The same for cairo_ctx_frame_rate, of a context with cairo_ctx_set_rate on
 * (turned on while the stream has no frame in flight; the stream's context
 * has CAIRO_OUT_FEED).  The frame record of the frame (quality included) is
 * the caller's to write: take the quality from here. */
CAIRO_API int cairo_stream_frame_rate(cairo_stream *s, int ticket, cairo_rate_info *out);
/* Finish all submitted frames and stop the threads. */
CAIRO_API int cairo_stream_destroy(cairo_stream *s);
/* Append n bits of src at bit *pos of dst (cap_bits), bit_stream semantics. */
CAIRO_API int cairo_bits_append(uint8_t *dst, uint64_t cap_bits, uint64_t *pos, const uint8_t *src,
                                uint64_t n);

/* ---- drop-in encoder, C view of evx1_encoder (evx1.h:66-94) ------------- */
CAIRO_API int evx_encoder_create(void **enc);
CAIRO_API int evx_encoder_destroy(void *enc);
CAIRO_API int evx_encoder_clear(void *enc);
CAIRO_API int evx_encoder_insert_intra(void *enc);
CAIRO_API int evx_encoder_set_quality(void *enc, uint8_t quality);
/* Encode one RGB888 frame, appending to the bit stream bs (evx_bitstream_*). */
CAIRO_API int evx_encoder_encode(void *enc, const void *rgb, uint32_t width, uint32_t height,
                                 void *bs);
/* Debug view of the last encoded frame (EVX_PEEK_STATE, evx1.h): RGB888 of
 * the nominal frame size into rgb (evx1enc.cpp:170-305). */
CAIRO_API int evx_encoder_peek(void *enc, int state, void *rgb);
CAIRO_API int evx_encoder_set_ring(void *enc, uint32_t ring); /* before first encode */
CAIRO_API int evx_encoder_set_device(void *enc, int device);  /* before first encode */
/* The layout encode() reads its image in from now on (CAIRO_FMT_*, row pitch
 * in bytes, 0: tight); callable between frames.  peek() keeps writing RGB888. */
CAIRO_API int evx_encoder_set_input_format(void *enc, int fmt, uint32_t pitch);
/* The colour description of the I420 / NV12 images encode() reads from now on
 * (cairo_ctx_set_input_color); callable between frames. */
CAIRO_API int evx_encoder_set_input_color(void *enc, int range, int matrix);
/* encode()'s image is, from now on, the address of element (0,0,0) of a tensor
 * in device memory of the encoder's GPU, read through desc
 * (cairo_ctx_submit_tensor; the frame size is still encode()'s width and
 * height).  desc == NULL goes back to the pixel formats.  Callable between
 * frames.  peek() is unchanged. */
CAIRO_API int evx_encoder_set_input_tensor(void *enc, const cairo_tensor *desc);
/* CAIRO_METRIC_* for the frames encode() codes from now on (callable between
 * frames), and the metrics of the last encoded frame (EVX_ERROR_INVALID_ARGS
 * when it has none). */
CAIRO_API int evx_encoder_set_metrics(void *enc, int flags);
CAIRO_API int evx_encoder_last_metrics(void *enc, cairo_frame_metrics *out);

/* ---- drop-in decoder, C view of evx1_decoder (evx1.h:97-112) ------------
 * decode() reads [header +] one frame record from bs (its read index onward),
 * writes the frame as RGB888 (width*height*3 from the stream header) to rgb,
 * and empties bs, as the reference does (evx1dec.cpp:90-124). */
CAIRO_API int evx_decoder_create(void **dec);
CAIRO_API int evx_decoder_destroy(void *dec);
CAIRO_API int evx_decoder_clear(void *dec);
CAIRO_API int evx_decoder_decode(void *dec, void *bs, void *rgb);
CAIRO_API int evx_decoder_set_device(void *dec, int device); /* before first decode */
/* The layout decode() writes its frame in from now on (CAIRO_FMT_*, row pitch
 * in bytes, 0: tight; cairo_frame_layout bytes); callable between frames. */
CAIRO_API int evx_decoder_set_output_format(void *dec, int fmt, uint32_t pitch);
/* The colour description decode() writes I420 / NV12 frames in from now on
 * (cairo_ctx_set_output_color); callable between frames. */
CAIRO_API int evx_decoder_set_output_color(void *dec, int range, int matrix);
/* decode()'s output is, from now on, the address of element (0,0,0) of a
 * tensor in device memory of the decoder's GPU, written through desc
 * (cairo_ctx_decode_frame_tensor).  desc == NULL goes back to the pixel
 * formats.  Callable between frames. */
CAIRO_API int evx_decoder_set_output_tensor(void *dec, const cairo_tensor *desc);

/* bit_stream (reference bitstream.h:43-92) */
CAIRO_API void *evx_bitstream_create(uint32_t size_in_bits);
CAIRO_API void evx_bitstream_destroy(void *bs);
CAIRO_API const uint8_t *evx_bitstream_data(void *bs);
CAIRO_API uint32_t evx_bitstream_occupancy(void *bs); /* bits */
CAIRO_API void evx_bitstream_empty(void *bs);
/* Append count bits of data (LSB-first) -- bit_stream::write_bits. */
CAIRO_API int evx_bitstream_write_bits(void *bs, const void *data, uint32_t count);

/* band4 synthetic content generator; RGB888, pitch 3*w. */
CAIRO_API void cairo_make_band4(uint8_t *rgb, uint32_t w, uint32_t h, uint32_t t, uint32_t seed);

/* Library/device information. */
CAIRO_API const char *cairo_version(void);
CAIRO_API int cairo_device_count(void);

#ifdef __cplusplus
}
#endif
#endif
