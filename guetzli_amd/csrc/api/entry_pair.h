// C ABI: the butteraugli distance of an image PAIR -- the context's original against pixels that are no JPEG candidate
// of it (gz_compare_device_pixels, gz_compare_rgb) -- and the distance map left on the device (gz_device_map,
// gz_distmap_device), written into the caller's strided device image by k_emit_map.
// (part of the one translation unit gz_api.hip, which includes these files in order -- no declaration here is visible
// outside libguetzli_amd.so but the C ABI)
#pragma once

extern "C" {

// k_emit_map on `stream`: plane (pitch floats per row) -> map (y, x: w x h, checked by the caller: check_device_map,
// tensor.h -- or one plane of a checked output).
static void launch_map(hipStream_t stream, const float* plane, int w, int h, int pitch, const TensorView& map) {
  const long long sy = map.dim[0].stride, sx = map.dim[1].stride;
  with_float_type(map.dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    launch_emit_map(stream, plane, w, h, pitch, (T*)map.data, sy, sx);
  });
}

// c->distmap -> map on the context's stream, under gz_device_output's stream contract in both directions (the
// consumer's stream is waited for before the kernel and waits for it afterwards).  Nothing is waited for on the host.
// win (may be NULL: the whole plane): the window of the plane that map, which is of ITS size, takes.
static int emit_distmap(gz_ctx* c, const gz_device_map* map, const MapWindow* win = nullptr) {
  TRY(outputs_after_consumers(c, c->stream, &c->ev_emit, {map->consumer_stream}));
  if (win) launch_map(c->stream, c->distmap + ((size_t)win->y0 * c->pitch + win->x0), win->w, win->h, c->pitch, tensor_view(map, win->w, win->h));
  else launch_map(c->stream, c->distmap, c->w, c->h, c->pitch, tensor_view(map, c->w, c->h));
  KCHK(c);
  TRY(consumers_after_outputs(c, c->stream, c->ev_emit, {map->consumer_stream}));
  return GZ_OK;
}

// What a pair comparison drops before its first copy or launch (context.h, DROP BEFORE WRITE): lin[] and xyb[] take the
// other image, the map and the block maxima are about to be replaced.  The candidate, the original and the frame stay.
static void pair_compare_drops(gz_ctx* c) {
  c->lin_is_cand = c->xyb_is_cand = false;
  c->have_distmap = c->h_block_max_valid = c->have_map_plane = false;
}

// lin[] holds the other image's linear planes: the chain from its second kernel on, as enqueue_compare runs it behind
// the reconstruction -- against pi0, the image maximum cleared by a fill -- then the map's two exits and the distance.
// heat (may be NULL): the map's heat map goes out behind the map itself; asking for it stores the map.
// lin (may be NULL; entry_linear.h): the other image came through k_ingest_linear, whose count rides home with the
// distance; with lin->win the images are smaller than the planes: map and heat map come from that window, and the
// distance is k_region_max's over it.
struct LinearTail {
  const MapWindow* win;
  uint64_t* clamped;   // (may be NULL)
};
static int pair_compare_tail(gz_ctx* c, float* distance, const gz_device_map* map, float* host_map, const HeatRequest* heat = nullptr,
                             const LinearTail* lin = nullptr) {
  const bool want_map = map != nullptr || host_map != nullptr || heat != nullptr || (lin && lin->win);   // (k_region_max reads the plane)
  const ChainStreams cs = chain_streams(c, !single_stream_wanted(c));
  TRY(stage_opsin(c, cs.main));
  TRY(stage_separate(c, cs, &c->pi1));
  TRY(stage_diffmap(c, cs, c->pi0, c->pi1, kWantBlockMax | (want_map ? kWantDistmap : 0u), ClearMax::kMemset));
  const MapWindow* win = lin ? lin->win : nullptr;
  if (map) TRY(emit_distmap(c, map, win));
  if (heat) TRY(emit_heat(c, *heat, win));
  if (win) {
    HIPCHK(c, hipMemsetAsync(c->d_max_bits + gz_ctx::kWordRegionMax, 0, sizeof(unsigned), c->stream));
    launch_region_max(c->stream, c->distmap, c->pitch, win->x0, win->y0, win->w, win->h, c->d_max_bits + gz_ctx::kWordRegionMax);
    KCHK(c);
  }
  const size_t fetched = lin ? sizeof(unsigned) * gz_ctx::kResultWords : 4;
  void* res = nullptr;
  TRY(result_buffer(c, fetched, &res));
  HIPCHK(c, hipMemcpyAsync(res, c->d_max_bits, fetched, hipMemcpyDeviceToHost, c->stream));
  if (host_map) TRY(download_plane(c, c->distmap, host_map));
  HIPCHK(c, hipStreamSynchronize(c->stream));   // (for the distance: the consumer of a map does not wait for this)
  memcpy(&c->last_distance, (const unsigned*)res + (win ? (int)gz_ctx::kWordRegionMax : 0), 4);
  if (lin && lin->clamped) *lin->clamped = ((const unsigned*)res)[gz_ctx::kWordClamped];
  *distance = c->last_distance;
  c->have_distmap = true;
  c->have_map_plane = want_map;
  return GZ_OK;
}

static int pair_compare_state(gz_ctx* c, const char* who) {
  if (c->pending.busy()) { c->err = std::string(who) + " while a Compare or phase-B work of the context is in flight"; return GZ_E_STATE; }
  return GZ_OK;
}

// gz_compare_device_pixels, and with heat != NULL gz_compare_device_pixels_heat.
static int compare_device_pixels(gz_ctx* c, const gz_device_pixels* other, float* distance, const gz_device_map* map, const HeatRequest* heat) {
  if (!c || !distance) return GZ_E_ARG;
  if (check_device_pixels(other, c->w, c->h) != GZ_OK) return GZ_E_ARG;   // (before any device call)
  if (map && check_device_map(map, c->w, c->h) != GZ_OK) return GZ_E_ARG;
  if (heat && check_heat_request(*heat, c->w, c->h) != GZ_OK) return GZ_E_ARG;
  DeviceScope ds_(c);
  if (const int rc = check_tensor_memory(c->device, tensor_view(other, c->w, c->h), "data", &c->err)) return rc;
  if (map)
    if (const int rc = check_tensor_memory(c->device, tensor_view(map, c->w, c->h), "map", &c->err)) return rc;
  if (heat)
    if (const int rc = check_tensor_memory(c->device, tensor_view(heat->out, c->w, c->h), "heat", &c->err)) return rc;
  TRY(pair_compare_state(c, heat ? "gz_compare_device_pixels_heat" : "gz_compare_device_pixels"));
  pair_compare_drops(c);
  TRY(wait_for_producer(c, other->producer_stream));
  // the packed bytes go to the reconstruction's scratch: d_rgb is the original's, and stays
  launch_ingest(c->stream, tensor_view(other, c->w, c->h), other->background, c->w, c->h, c->d_srgb_out, c->d_srgb_lut, c->lin[0], c->pitch, c->plane);
  KCHK(c);
  return pair_compare_tail(c, distance, map, nullptr, heat);   // (its synchronise: `other` is read when the call returns)
}

int gz_compare_device_pixels(gz_ctx* c, const gz_device_pixels* other, float* distance, const gz_device_map* map) {
  return compare_device_pixels(c, other, distance, map, nullptr);
}

int gz_compare_device_pixels_heat(gz_ctx* c, const gz_device_pixels* other, float* distance, const gz_device_map* map,
                                  const gz_device_output* heat, double good, double bad) {
  const HeatRequest req{heat, good, bad};
  return compare_device_pixels(c, other, distance, map, heat ? &req : nullptr);
}

int gz_compare_rgb(gz_ctx* c, const uint8_t* host_rgb, float* distance, float* host_distmap) {
  DeviceScope ds_(c);
  if (!c || !host_rgb || !distance) return GZ_E_ARG;
  TRY(pair_compare_state(c, "gz_compare_rgb"));
  pair_compare_drops(c);
  HIPCHK(c, hipMemcpyAsync(c->d_srgb_out, host_rgb, (size_t)3 * c->w * c->h, hipMemcpyHostToDevice, c->stream));
  GZ_LAUNCH(k_linear_from_rgb8, dim3(gz_div_up(c->w, 256), c->h), dim3(256), c->stream, c->d_srgb_out, c->w, c->h, c->pitch,
            c->plane, c->d_srgb_lut, c->lin[0]);
  KCHK(c);
  return pair_compare_tail(c, distance, nullptr, host_distmap);
}

int gz_distmap_device(gz_ctx* c, const gz_device_map* map) {
  if (!c) return GZ_E_ARG;
  if (check_device_map(map, c->w, c->h) != GZ_OK) return GZ_E_ARG;
  DeviceScope ds_(c);
  if (const int rc = check_tensor_memory(c->device, tensor_view(map, c->w, c->h), "map", &c->err)) return rc;
  if (!c->have_map_plane) { c->err = "the last comparison stored no distance map"; return GZ_E_STATE; }
  TRY(emit_distmap(c, map));
  if (map->consumer_stream) return GZ_OK;   // (ordered on the device: nothing to wait for here)
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GZ_OK;
}

#ifndef GZ_NO_PROBES
namespace {
struct ProbeMapScratch {   // the plane from the device pool and a pooled event (t: its record), given back on every path
  gz_ctx t;
  void* plane = nullptr;
  hipEvent_t ev = nullptr;
  ~ProbeMapScratch() { pool_free(plane); release_owned(&t); }
};
int probe_emit_map(int device, const float* host_plane, int w, int h, const gz_device_map* map) {
  if (probe_device(device) != GZ_OK) return GZ_E_NO_DEVICE;
  if (check_tensor_memory(device, tensor_view(map, w, h), "map", nullptr) != GZ_OK) return GZ_E_ARG;
  ProbeMapScratch s;
  const size_t bytes = sizeof(float) * (size_t)w * h;
  {
    const hipError_t e = pool_malloc(&s.plane, bytes);
    if (e != hipSuccess) { s.plane = nullptr; (void)hipGetLastError(); return e == hipErrorOutOfMemory ? GZ_E_NOMEM : GZ_E_HIP; }
  }
  const hipStream_t stream = (hipStream_t)0;
  if (hipMemcpy(s.plane, host_plane, bytes, hipMemcpyHostToDevice) != hipSuccess) return GZ_E_HIP;
  if (outputs_after_consumers(&s.t, stream, &s.ev, {map->consumer_stream}) != GZ_OK) return GZ_E_HIP;
  launch_map(stream, (const float*)s.plane, w, h, w, tensor_view(map, w, h));
  int rc = hipGetLastError() == hipSuccess ? GZ_OK : GZ_E_HIP;
  if (rc == GZ_OK && consumers_after_outputs(&s.t, stream, s.ev, {map->consumer_stream}) != GZ_OK) rc = GZ_E_HIP;
  if (hipStreamSynchronize(stream) != hipSuccess) rc = GZ_E_HIP;   // (the plane goes back to the pool behind this)
  return rc;
}
}  // namespace

int gz_probe_emit_map(int device, const float* host_plane, int w, int h, const gz_device_map* map) {
  if (!host_plane || check_device_map(map, w, h) != GZ_OK) return GZ_E_ARG;   // (before any device call)
  CallerDevice keep(device);
  return probe_emit_map(device, host_plane, w, h, map);
}
#endif  // GZ_NO_PROBES

}  // extern "C"
