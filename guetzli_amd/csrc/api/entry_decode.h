// C ABI: device-resident output -- OutputImage::ToSRGB of coefficients without a context (gz_decode_coeffs*), and of a
// context's candidate (gz_reconstruct_device), written into the caller's strided device image by k_emit_rgb.
// (part of the one translation unit gz_api.hip, which includes these files in order -- no declaration here is visible
// outside libguetzli_amd.so but the C ABI)
#pragma once

extern "C" {

// The arguments alone: no device call (the library answers these without a GPU).
static int check_device_output(const gz_device_output* out, int w, int h) {
  if (!out || out->struct_size != (int)sizeof(gz_device_output) || !out->data) return GZ_E_ARG;
  if (out->dtype < GZ_DT_U8 || out->dtype > GZ_DT_U16) return GZ_E_ARG;
  if (out->stride_y < 0 || out->stride_x < 0 || out->stride_c < 0) return GZ_E_ARG;
  if (w <= 0 || h <= 0 || w >= (1 << 16) || h >= (1 << 16)) return GZ_E_ARG;
  // the last element's offset (h-1) sy + (w-1) sx + 2 sc in 62 bits: every term is bounded before it is formed
  const uint64_t lim = (1ull << 62) - 1;
  const uint64_t sy = (uint64_t)out->stride_y, sx = (uint64_t)out->stride_x, sc = (uint64_t)out->stride_c;
  if ((h > 1 && sy > lim / (uint64_t)(h - 1)) || (w > 1 && sx > lim / (uint64_t)(w - 1)) || sc > lim / 2) return GZ_E_ARG;
  const uint64_t ty = sy * (uint64_t)(h - 1), tx = sx * (uint64_t)(w - 1), tc = sc * 2;   // each <= lim < 2^62
  if (ty + tx > lim || ty + tx + tc > lim) return GZ_E_ARG;
  // No two of the w * h * 3 elements at one address.  Sufficient: the dimensions ordered by stride, each stride at
  // least the extent stride * count of the one before -- and at least 1: a stride of 0, a convenience of the input
  // side, would make the kernel's lanes write one element in turns.  A dimension of one element addresses nothing:
  // its stride does not count.  (stride * count <= 2 lim: no overflow)
  std::pair<uint64_t, uint64_t> dim[3] = {{sy, (uint64_t)h}, {sx, (uint64_t)w}, {sc, 3}};
  std::sort(dim, dim + 3);
  uint64_t least = 1;
  for (const auto& d : dim) {
    if (d.second == 1) continue;
    if (d.first < least) return GZ_E_ARG;
    least = d.first * d.second;
  }
  return GZ_OK;
}

static uint64_t device_output_last(const gz_device_output* out, int w, int h) {
  return (uint64_t)out->stride_y * (uint64_t)(h - 1) + (uint64_t)out->stride_x * (uint64_t)(w - 1) + (uint64_t)out->stride_c * 2;
}

// k_emit_rgb on `stream`: rgb [h][w][3] -> out (checked by the caller); lut: emit_lut() in device memory.
static void launch_emit(hipStream_t stream, const uint8_t* rgb, int w, int h, const gz_device_output* out, const float* lut) {
  const long long sy = out->stride_y, sx = out->stride_x, sc = out->stride_c;
  switch (out->dtype) {
    case GZ_DT_U8: launch_emit_rgb(stream, rgb, w, h, (uint8_t*)out->data, sy, sx, sc, lut); break;
    case GZ_DT_F32: launch_emit_rgb(stream, rgb, w, h, (float*)out->data, sy, sx, sc, lut); break;
    case GZ_DT_F16: launch_emit_rgb(stream, rgb, w, h, (ingest_f16*)out->data, sy, sx, sc, lut); break;
    case GZ_DT_BF16: launch_emit_rgb(stream, rgb, w, h, (ingest_bf16*)out->data, sy, sx, sc, lut); break;
    default: launch_emit_rgb(stream, rgb, w, h, (uint16_t*)out->data, sy, sx, sc, lut); break;
  }
}

// The stream contract of gz_device_output around the emit kernel on `stream`, with the event `ev`:
// before: `stream` waits for what the consumer's stream has been given so far (a caching allocator may have handed the
// memory out while earlier work of that stream still uses it); behind: the consumer's stream waits for the kernel.
static hipError_t emit_after_consumer(hipStream_t stream, hipEvent_t ev, void* consumer) {
  const hipError_t e = hipEventRecord(ev, (hipStream_t)consumer);
  return e != hipSuccess ? e : hipStreamWaitEvent(stream, ev, 0);
}
static hipError_t consumer_after_emit(hipStream_t stream, hipEvent_t ev, void* consumer) {
  const hipError_t e = hipEventRecord(ev, stream);
  return e != hipSuccess ? e : hipStreamWaitEvent((hipStream_t)consumer, ev, 0);
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
};

// coeffs (host, frame layout of `chroma_factor`) -> the packed image on the device -> out and / or host_rgb.
int decode_coeffs(int device, const int16_t* coeffs, int w, int h, int chroma_factor, const gz_device_output* out,
                  uint8_t* host_rgb) {
  if (probe_device(device) != GZ_OK) return GZ_E_NO_DEVICE;
  if (out && check_device_range(device, out->data, device_output_last(out, w, h), ingest_elem_size(out->dtype), "data", nullptr) != GZ_OK)
    return GZ_E_ARG;
  DecodeScratch s;
  gz_ctx* c = &s.t;
  c->device = device;
  c->w = w; c->h = h;
  c->bw = (w + 7) / 8; c->bh = (h + 7) / 8; c->nb = c->bw * c->bh;
  c->pitch = w;
  c->plane = (size_t)w * h;
  set_frame(c, chroma_factor);
  // the coefficients, the packed pixels, the table, and (4:2:0) the chroma samples stage_reconstruct would otherwise
  // make on its own: all of them or none
  if (chroma_factor == 2) {
    TRY(regrow(c, nullptr, nullptr, 0, {{(void**)&c->d_cand, (size_t)c->nblk * 128}, {(void**)&c->d_srgb_out, (size_t)3 * w * h},
                                        {(void**)&s.d_lut, sizeof(float) * 256}, {(void**)&c->d_csamp, 2 * csamp_plane(c)}}));
  } else {
    TRY(regrow(c, nullptr, nullptr, 0, {{(void**)&c->d_cand, (size_t)c->nblk * 128}, {(void**)&c->d_srgb_out, (size_t)3 * w * h},
                                        {(void**)&s.d_lut, sizeof(float) * 256}}));
  }
  {
    const hipError_t e = pool_stream_set_create(&s.ss, false, 0);
    s.have_streams = e == hipSuccess;
    if (e != hipSuccess) { stream_set_teardown(s.ss); s.ss = StreamSet(); (void)hipGetLastError(); return e == hipErrorOutOfMemory ? GZ_E_NOMEM : GZ_E_HIP; }
  }
  const hipStream_t stream = s.ss.own;
  s.idle = false;
  if (out && out->consumer_stream) {
    TRY(own_event(c, &s.ev));
    HIPCHK(c, emit_after_consumer(stream, s.ev, out->consumer_stream));
  }
  HIPCHK(c, hipMemcpyAsync(c->d_cand, coeffs, (size_t)c->nblk * 128, hipMemcpyHostToDevice, stream));
  TRY(stage_reconstruct(c, stream, c->d_cand, nullptr, c->d_srgb_out));
  if (out) {
    if (out->dtype != GZ_DT_U8 && out->dtype != GZ_DT_U16)
      HIPCHK(c, hipMemcpyAsync(s.d_lut, emit_lut(), sizeof(float) * 256, hipMemcpyHostToDevice, stream));
    launch_emit(stream, c->d_srgb_out, w, h, out, s.d_lut);
    KCHK(c);
    if (out->consumer_stream) HIPCHK(c, consumer_after_emit(stream, s.ev, out->consumer_stream));
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
  int prev = -1;
  if (hipGetDevice(&prev) != hipSuccess) { (void)hipGetLastError(); prev = -1; }
  const int rc = decode_coeffs(device, coeffs, w, h, chroma_factor, out, host_rgb);
  if (prev >= 0 && prev != device) (void)hipSetDevice(prev);   // the caller's device stays current
  return rc;
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
  if (const int rc = check_device_range(c->device, out->data, device_output_last(out, c->w, c->h), ingest_elem_size(out->dtype), "data", &c->err)) return rc;
  if (!c->made.emit) {
    TRY(regrow(c, c->stream, nullptr, 0, {{(void**)&c->d_emit_lut, sizeof(float) * 256}}));
    HIPCHK(c, hipMemcpyAsync(c->d_emit_lut, emit_lut(), sizeof(float) * 256, hipMemcpyHostToDevice, c->stream));
    c->made.emit = true;
  }
  if (out->consumer_stream) {
    if (!c->ev_emit) TRY(own_event(c, &c->ev_emit));
    HIPCHK(c, emit_after_consumer(c->stream, c->ev_emit, out->consumer_stream));
  }
  TRY(stage_reconstruct(c, c->stream, c->d_cand, nullptr, c->d_srgb_out));
  launch_emit(c->stream, c->d_srgb_out, c->w, c->h, out, c->d_emit_lut);
  KCHK(c);
  if (out->consumer_stream) {
    HIPCHK(c, consumer_after_emit(c->stream, c->ev_emit, out->consumer_stream));
    return GZ_OK;   // (ordered on the device: nothing to wait for here)
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GZ_OK;
}

}  // extern "C"
