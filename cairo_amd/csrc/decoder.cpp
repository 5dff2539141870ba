// cairo_amd/csrc/decoder.cpp -- the drop-in evx1_decoder (reference
// evx1dec.cpp:13-136, evx1.cpp:28-81, decode.cpp:146-198) on top of the GPU
// backend.
//
// decode(): lazy init from the stream header, frame descriptor, host entropy
// decode (unserialize_slice, into the persistent block table and coefficient
// planes), the table's legality (cairo_table_check: a table the engine cannot
// honour is an error), then the GPU hot path (cairo_ctx_decode_frame: the
// decode-mode engine reconstructs and deblocks the frame into its ring slot,
// and convert_image writes RGB888), then the reference's frame-state update.
// Like the reference, decode consumes the caller's bit_stream and empties it.
#include <cstdlib>
#include <cstring>
#include <new>

#include "../../include/cairo_amd.h"
#include "../../include/evx1.h"
#include "evx_defs.h"
#include "frame_io.h"
#include "stream_format.h"

namespace cairo {
int unserialize_slice(const uint8_t* data, uint32_t* read_index, uint32_t write_index, uint32_t wmb,
                      uint32_t hmb, uint32_t ring, BlockDesc* table, int16_t* cy, int16_t* cu, int16_t* cv);
}

namespace evx {

class gpu_decoder : public evx1_decoder {
 public:
  gpu_decoder() { frame_index_ = 0; }
  ~gpu_decoder() override { clear(); }

  evx_status clear() override {  // evx1dec.cpp:27-41
    if (!initialized_) return EVX_SUCCESS;
    cairo_ctx_destroy(ctx_);
    ctx_ = nullptr;
    free(table_);
    free(coef_);
    table_ = nullptr;
    coef_ = nullptr;
    frame_index_ = 0;
    initialized_ = false;
    return EVX_SUCCESS;
  }

  evx_status decode(bit_stream *input, void *output) override {  // evx1dec.cpp:90-124
    if (!input || !output) return EVX_ERROR_INVALIDARG;
    if (!initialized_ && initialize(input) != EVX_SUCCESS) return EVX_ERROR_EXECUTION_FAILURE;
    frame_t f;  // read_frame_desc (evx1dec.cpp:75-88)
    if (input->read_bytes(&f, sizeof(f)) != EVX_SUCCESS || f.index != frame_index_)
      return EVX_ERROR_EXECUTION_FAILURE;
    uint32 rd = input->query_read_index();
    const size_t ny = (size_t)wa_ * ha_, nc = ny / 4;
    if (cairo::unserialize_slice(input->query_data(), &rd, input->query_write_index(), wmb_, hmb_,
                                 ring_, table_, coef_, coef_ + ny, coef_ + ny + nc))
      return EVX_ERROR_EXECUTION_FAILURE;
    input->set_read_index(rd);
    const uint8_t *tbl = reinterpret_cast<const uint8_t *>(table_);
    // the engine trusts the table: a stream it cannot honour is an error
    if (!cairo_table_check(tbl, wmb_, hmb_, ring_)) return EVX_ERROR_EXECUTION_FAILURE;
    if (cairo::decode_frame(ctx_, tbl, coef_, f.index, out_.sink(output))) return EVX_ERROR_EXECUTION_FAILURE;
    frame_index_++;
    input->empty();
    return EVX_SUCCESS;
  }

  evx_status set_device(int device) {
    if (initialized_) return EVX_ERROR_INVALIDARG;
    device_ = device;
    return EVX_SUCCESS;
  }
  // The layout decode() writes its frame in (between frames too).
  evx_status set_output_format(int fmt, uint32 pitch) {
    // (the frame size is known once initialised; clear() forgets it)
    const bool ok = out_.set_format(fmt, pitch, initialized_ ? width_ : 0, initialized_ ? height_ : 0);
    return ok ? EVX_SUCCESS : EVX_ERROR_INVALIDARG;
  }
  // decode()'s output as a device tensor written through desc (between frames
  // too; nullptr: back to the pixel formats).  Its strides are checked against
  // the frame size at each decode().
  evx_status set_output_tensor(const cairo_tensor *desc) {
    return out_.set_tensor(desc) ? EVX_SUCCESS : EVX_ERROR_INVALIDARG;
  }
  // The colour description decode() writes I420 / NV12 frames in (between
  // frames too; RGB frames ignore it).
  evx_status set_output_color(int range, int matrix) {
    const bool ok = out_.set_color(1, range, matrix, initialized_ ? ctx_ : nullptr);
    return ok ? EVX_SUCCESS : EVX_ERROR_INVALIDARG;
  }

 private:
  // initialize (evx1dec.cpp:43-73) with verify_header (common.cpp:25-43).  The
  // reference compiles its ring size in; this decoder takes it from the
  // header (2..4, the sizes the encoder supports).
  evx_status initialize(bit_stream *input) {
    header_t h;
    memset(&h, 0, sizeof(h));
    input->read_bytes(&h, sizeof(h));
    if (h.magic[0] != 'E' || h.magic[1] != 'V' || h.magic[2] != 'X' || h.magic[3] != '1' ||
        h.version != kVersionWord || h.size != sizeof(header_t) || h.ref_count < 2 ||
        h.ref_count > (uint8)cairo::kMaxRing || !h.frame_width || !h.frame_height ||
        (h.frame_width & 1) || (h.frame_height & 1))  // convert_image needs even sizes (convert.cpp:195-199)
      return EVX_ERROR_INVALID_RESOURCE;
    width_ = h.frame_width;
    height_ = h.frame_height;
    ring_ = h.ref_count;
    wa_ = (width_ + 15) & ~15u;
    ha_ = (height_ + 15) & ~15u;
    wmb_ = wa_ / 16;
    hmb_ = ha_ / 16;
    if (cairo_ctx_create_ex(width_, height_, ring_, device_, 2, &ctx_)) return EVX_ERROR_HARDWAREFAIL;  // synchronous: 2 slots
    (void)cairo_ctx_set_output_color(ctx_, out_.range, out_.matrix);  // (checked by set_output_color)
    table_ = (cairo::BlockDesc *)calloc((size_t)wmb_ * hmb_, sizeof(cairo::BlockDesc));
    coef_ = (int16 *)calloc((size_t)wa_ * ha_ * 3 / 2, sizeof(int16));
    if (!table_ || !coef_) {
      free(table_);
      free(coef_);
      cairo_ctx_destroy(ctx_);
      ctx_ = nullptr;
      table_ = nullptr;
      coef_ = nullptr;
      return EVX_ERROR_OUTOFMEMORY;
    }
    frame_index_ = 0;
    initialized_ = true;
    return EVX_SUCCESS;
  }

  bool initialized_ = false;
  uint32 frame_index_;
  uint32 width_ = 0, height_ = 0, wa_ = 0, ha_ = 0, wmb_ = 0, hmb_ = 0, ring_ = 0;
  int device_ = 0;
  cairo::FrameIo out_;  // decode()'s output (set_output_format / _tensor / _color)
  cairo_ctx *ctx_ = nullptr;
  cairo::BlockDesc *table_ = nullptr;
  int16 *coef_ = nullptr;
};

evx_status create_decoder(evx1_decoder **output) {  // evx1.cpp:28-45
  if (!output) return EVX_ERROR_INVALIDARG;
  *output = new (std::nothrow) gpu_decoder;
  return *output ? EVX_SUCCESS : EVX_ERROR_OUTOFMEMORY;
}

evx_status destroy_decoder(evx1_decoder *input) {  // evx1.cpp:65-81
  if (!input) return EVX_ERROR_INVALIDARG;
  delete static_cast<gpu_decoder *>(input);
  return EVX_SUCCESS;
}

}  // namespace evx

extern "C" {

int evx_decoder_create(void **dec) {
  evx::evx1_decoder *d = nullptr;
  const int r = evx::create_decoder(&d);
  *dec = d;
  return r;
}
int evx_decoder_destroy(void *dec) { return evx::destroy_decoder((evx::evx1_decoder *)dec); }
int evx_decoder_clear(void *dec) { return ((evx::evx1_decoder *)dec)->clear(); }
int evx_decoder_decode(void *dec, void *bs, void *rgb) {
  return ((evx::evx1_decoder *)dec)->decode((evx::bit_stream *)bs, rgb);
}
int evx_decoder_set_device(void *dec, int device) {
  return static_cast<evx::gpu_decoder *>((evx::evx1_decoder *)dec)->set_device(device);
}
int evx_decoder_set_output_format(void *dec, int fmt, uint32_t pitch) {
  return static_cast<evx::gpu_decoder *>((evx::evx1_decoder *)dec)->set_output_format(fmt, pitch);
}
int evx_decoder_set_output_tensor(void *dec, const cairo_tensor *desc) {
  return static_cast<evx::gpu_decoder *>((evx::evx1_decoder *)dec)->set_output_tensor(desc);
}
int evx_decoder_set_output_color(void *dec, int range, int matrix) {
  return static_cast<evx::gpu_decoder *>((evx::evx1_decoder *)dec)->set_output_color(range, matrix);
}

}  // extern "C"
