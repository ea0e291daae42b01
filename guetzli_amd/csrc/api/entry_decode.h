// C ABI: device-resident output -- OutputImage::ToSRGB of coefficients without a context (gz_decode_coeffs*), and of a
// context's candidate (gz_reconstruct_device), written into the caller's strided device image by k_emit_rgb.
// (part of the one translation unit gz_api.hip, which includes these files in order -- no declaration here is visible
// outside libguetzli_amd.so but the C ABI)
#pragma once

extern "C" {

// k_emit_rgb on `stream`: rgb [h][w][3] -> out (checked by the caller: check_device_output, tensor.h); lut: emit_lut() in
// device memory.
static void launch_emit(hipStream_t stream, const uint8_t* rgb, int w, int h, const gz_device_output* out, const float* lut) {
  const long long sy = out->stride_y, sx = out->stride_x, sc = out->stride_c;
  with_sample_type(out->dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    launch_emit_rgb(stream, rgb, w, h, (T*)out->data, sy, sx, sc, lut);
  });
}

namespace {
// What a context-free decode holds for the length of the call: a bare gz_ctx as the owner's record of its device
// memory and its event -- regrow() / own_event() / release_owned(), the all-or-nothing ownership of a context, from the
// same pools -- and a stream set of the pool, of which the main stream does the work.  Nothing else of the gz_ctx is
// used but the geometry stage_reconstruct reads.
struct DecodeScratch {
  gz_ctx t;
  StreamSet ss;
  float* d_lut = nullptr;
  uint8_t* d_scan = nullptr;   // gz_decode_scan*: the scan decoder's scratch (entry_scandec.h)
  hipEvent_t ev = nullptr;
  bool have_streams = false;
  bool idle = true;   // nothing enqueued that has not been waited for
  DecodeScratch() = default;
  DecodeScratch(const DecodeScratch&) = delete;
  DecodeScratch& operator=(const DecodeScratch&) = delete;
  ~DecodeScratch() {
    // everything enqueued must be done before the memory goes back to the pool, which hands it on without waiting
    if (ss.own && !idle) (void)hipStreamSynchronize(ss.own);
    release_owned(&t);
    if (have_streams) pool_stream_set_destroy(ss, false, 0);
  }
  // The geometry of a w x h frame of `chroma_factor`, for stage_reconstruct.
  void set_frame_geometry(int device, int w, int h, int chroma_factor) {
    t.device = device;
    t.w = w; t.h = h;
    t.bw = (w + 7) / 8; t.bh = (h + 7) / 8; t.nb = t.bw * t.bh;
    t.pitch = w;
    t.plane = (size_t)w * h;
    set_frame(&t, chroma_factor);
  }
  // The stream set of the pool; work goes onto *stream, its main stream, from here on.
  int open_streams(hipStream_t* stream) {
    const hipError_t e = pool_stream_set_create(&ss, false, 0);
    have_streams = e == hipSuccess;
    if (e != hipSuccess) { stream_set_teardown(ss); ss = StreamSet(); (void)hipGetLastError(); return e == hipErrorOutOfMemory ? GZ_E_NOMEM : GZ_E_HIP; }
    *stream = ss.own;
    idle = false;
    return GZ_OK;
  }
};

// coeffs (host, frame layout of `chroma_factor`) -> the packed image on the device -> out and / or host_rgb.
int decode_coeffs(int device, const int16_t* coeffs, int w, int h, int chroma_factor, const gz_device_output* out,
                  uint8_t* host_rgb) {
  if (probe_device(device) != GZ_OK) return GZ_E_NO_DEVICE;
  if (out && check_tensor_memory(device, tensor_view(out, w, h), "data", nullptr) != GZ_OK) return GZ_E_ARG;
  DecodeScratch s;
  gz_ctx* c = &s.t;
  s.set_frame_geometry(device, w, h, chroma_factor);
  // the coefficients, the packed pixels, the table, and (4:2:0) the chroma samples stage_reconstruct would otherwise
  // make on its own: all of them or none
  if (chroma_factor == 2) {
    TRY(regrow(c, nullptr, nullptr, 0, {{(void**)&c->d_cand, (size_t)c->nblk * 128}, {(void**)&c->d_srgb_out, (size_t)3 * w * h},
                                        {(void**)&s.d_lut, sizeof(float) * 256}, {(void**)&c->d_csamp, 2 * csamp_plane(c)}}));
  } else {
    TRY(regrow(c, nullptr, nullptr, 0, {{(void**)&c->d_cand, (size_t)c->nblk * 128}, {(void**)&c->d_srgb_out, (size_t)3 * w * h},
                                        {(void**)&s.d_lut, sizeof(float) * 256}}));
  }
  hipStream_t stream = nullptr;
  TRY(s.open_streams(&stream));
  if (out) TRY(outputs_after_consumers(c, stream, &s.ev, {out->consumer_stream}));
  HIPCHK(c, hipMemcpyAsync(c->d_cand, coeffs, (size_t)c->nblk * 128, hipMemcpyHostToDevice, stream));
  TRY(stage_reconstruct(c, stream, c->d_cand, nullptr, c->d_srgb_out));
  if (out) {
    if (tensor_float_dtype(out->dtype))
      HIPCHK(c, hipMemcpyAsync(s.d_lut, emit_lut(), sizeof(float) * 256, hipMemcpyHostToDevice, stream));
    launch_emit(stream, c->d_srgb_out, w, h, out, s.d_lut);
    KCHK(c);
    TRY(consumers_after_outputs(c, stream, s.ev, {out->consumer_stream}));
  }
  if (host_rgb) HIPCHK(c, hipMemcpyAsync(host_rgb, c->d_srgb_out, (size_t)3 * w * h, hipMemcpyDeviceToHost, stream));
  HIPCHK(c, hipStreamSynchronize(stream));   // (the temporaries go back to the pool behind this)
  s.idle = true;
  return GZ_OK;
}

int decode_coeffs_entry(int device, const int16_t* coeffs, int w, int h, int chroma_factor, const gz_device_output* out,
                        uint8_t* host_rgb) {
  if (!coeffs || (chroma_factor != 1 && chroma_factor != 2)) return GZ_E_ARG;
  if (w <= 0 || h <= 0 || w >= (1 << 16) || h >= (1 << 16)) return GZ_E_ARG;
  if ((uint64_t)((w + 7) / 8) * (uint64_t)((h + 7) / 8) * 192u > 0x7fffffffull) return GZ_E_ARG;   // gz_create's block limit
  CallerDevice keep(device);
  return decode_coeffs(device, coeffs, w, h, chroma_factor, out, host_rgb);
}
}  // namespace

int gz_decode_coeffs_device(int device, const int16_t* coeffs, int w, int h, int chroma_factor, const gz_device_output* out) {
  if (check_device_output(out, w, h) != GZ_OK) return GZ_E_ARG;   // (before any device call)
  return decode_coeffs_entry(device, coeffs, w, h, chroma_factor, out, nullptr);
}

int gz_decode_coeffs(int device, const int16_t* coeffs, int w, int h, int chroma_factor, uint8_t* host_rgb_out) {
  if (!host_rgb_out) return GZ_E_ARG;
  return decode_coeffs_entry(device, coeffs, w, h, chroma_factor, nullptr, host_rgb_out);
}

int gz_reconstruct_device(gz_ctx* c, const gz_device_output* out) {
  if (!c) return GZ_E_ARG;
  if (check_device_output(out, c->w, c->h) != GZ_OK) return GZ_E_ARG;
  DeviceScope ds_(c);
  if (!c->have_cand) { c->err = "no candidate coefficients"; return GZ_E_STATE; }
  if (const int rc = check_tensor_memory(c->device, tensor_view(out, c->w, c->h), "data", &c->err)) return rc;
  if (!c->made.emit) {
    TRY(regrow(c, c->stream, nullptr, 0, {{(void**)&c->d_emit_lut, sizeof(float) * 256}}));
    HIPCHK(c, hipMemcpyAsync(c->d_emit_lut, emit_lut(), sizeof(float) * 256, hipMemcpyHostToDevice, c->stream));
    c->made.emit = true;
  }
  TRY(outputs_after_consumers(c, c->stream, &c->ev_emit, {out->consumer_stream}));
  TRY(stage_reconstruct(c, c->stream, c->d_cand, nullptr, c->d_srgb_out));
  launch_emit(c->stream, c->d_srgb_out, c->w, c->h, out, c->d_emit_lut);
  KCHK(c);
  TRY(consumers_after_outputs(c, c->stream, c->ev_emit, {out->consumer_stream}));
  if (out->consumer_stream) return GZ_OK;   // (ordered on the device: nothing to wait for here)
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GZ_OK;
}

}  // extern "C"
