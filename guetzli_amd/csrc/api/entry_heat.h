// C ABI: butteraugli's heat map on the device -- CreateHeatMapImage (butteraugli.cc:1979-1992) of a context's stored
// distance map (gz_heatmap_device; gz_compare_device_pixels_heat in entry_pair.h) or of a float plane of the caller's
// (gz_heatmap_from_map_device), written into the caller's strided device image by k_emit_heat -- and the two functions
// its default thresholds come from (gz_butteraugli_fuzzy_class / gz_butteraugli_fuzzy_inverse).
// (part of the one translation unit gz_api.hip, which includes these files in order -- no declaration here is visible
// outside libguetzli_amd.so but the C ABI)
#pragma once

extern "C" {

// ButteraugliFuzzyClass / ButteraugliFuzzyInverse (butteraugli.cc:1903-1934), with the host's exp: no device call.
double gz_butteraugli_fuzzy_class(double score) {
  static const double fuzzy_width_up = 6.07887388532;
  static const double fuzzy_width_down = 5.50793514384;
  static const double m0 = 2.0;
  static const double scaler = 0.840253347958;
  double val;
  if (score < 1.0) {
    val = m0 / (1.0 + exp((score - 1.0) * fuzzy_width_down));
    val -= 1.0;
    val *= 2.0 - scaler;
    val += scaler;
  } else {
    val = m0 / (1.0 + exp((score - 1.0) * fuzzy_width_up));
    val *= scaler;
  }
  return val;
}

double gz_butteraugli_fuzzy_inverse(double seek) {
  double pos = 0;
  for (double range = 1.0; range >= 1e-10; range *= 0.5) {
    const double cur = gz_butteraugli_fuzzy_class(pos);
    if (cur < seek) pos -= range;
    else pos += range;
  }
  return pos;
}

// A heat map asked for: where it goes and the two thresholds of ScoreToRgb.
struct HeatRequest {
  const gz_device_output* out;
  double good, bad;
};

// The arguments alone: no device call.  0 < good < bad, both finite (NaN fails every comparison).
static int check_heat_request(const HeatRequest& heat, int w, int h) {
  if (!(heat.good > 0.0 && heat.good < heat.bad && heat.bad < INFINITY)) return GZ_E_ARG;
  return check_device_output(heat.out, w, h);
}

// What k_emit_heat reads from device memory, in one block: emit_lut()'s 256 floats, then the 255 thresholds.
static const size_t kHeatTabBytes = sizeof(float) * 256 + sizeof(double) * 255;
static const double* heat_tab_thresholds(const float* tab) { return reinterpret_cast<const double*>(tab + 256); }
static hipError_t upload_heat_tab(float* tab, hipStream_t stream) {
  const hipError_t e = hipMemcpyAsync(tab, emit_lut(), sizeof(float) * 256, hipMemcpyHostToDevice, stream);
  return e != hipSuccess ? e : hipMemcpyAsync(tab + 256, heat_thresholds().thr, sizeof(double) * 255, hipMemcpyHostToDevice, stream);
}

// k_emit_heat on `stream`: plane (pitch floats per row) -> heat.out (checked by the caller); tab: upload_heat_tab's.
static void launch_heat(hipStream_t stream, const float* plane, int w, int h, int pitch, const HeatRequest& heat, const float* tab) {
  const gz_device_output* out = heat.out;
  const long long sy = out->stride_y, sx = out->stride_x, sc = out->stride_c;
  const double* thr = heat_tab_thresholds(tab);
  const HeatScale hs = heat_scale(heat.good, heat.bad);
  with_sample_type(out->dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    launch_emit_heat(stream, plane, w, h, pitch, (T*)out->data, sy, sx, sc, tab, thr, hs);
  });
}

// A window of the context's map plane: w x h from (x0, y0) on.  What a map and its heat map are emitted from where the
// image is smaller than the plane (gz_butteraugli_linear under 8 pixels: the reference's crop, butteraugli.cc:1846-1854).
struct MapWindow {
  int x0, y0, w, h;
};

// c->distmap -> heat.out on the context's stream, under gz_device_output's stream contract in both directions, as
// emit_distmap writes the map itself.  Nothing is waited for on the host, no claim of the context changes.
// win (may be NULL: the whole plane): the window heat.out, which is of ITS size, takes.
static int emit_heat(gz_ctx* c, const HeatRequest& heat, const MapWindow* win = nullptr) {
  if (!heat_thresholds().ok) { c->err = heat_thresholds().why; return GZ_E_STATE; }
  if (!c->made.heat) {
    TRY(regrow(c, c->stream, nullptr, 0, {{(void**)&c->d_heat_tab, kHeatTabBytes}}));
    HIPCHK(c, upload_heat_tab(c->d_heat_tab, c->stream));
    c->made.heat = true;
  }
  TRY(outputs_after_consumers(c, c->stream, &c->ev_emit, {heat.out->consumer_stream}));
  if (win) launch_heat(c->stream, c->distmap + ((size_t)win->y0 * c->pitch + win->x0), win->w, win->h, c->pitch, heat, c->d_heat_tab);
  else launch_heat(c->stream, c->distmap, c->w, c->h, c->pitch, heat, c->d_heat_tab);
  KCHK(c);
  TRY(consumers_after_outputs(c, c->stream, c->ev_emit, {heat.out->consumer_stream}));
  return GZ_OK;
}

int gz_heatmap_device(gz_ctx* c, double good, double bad, const gz_device_output* out) {
  if (!c) return GZ_E_ARG;
  const HeatRequest heat{out, good, bad};
  if (check_heat_request(heat, c->w, c->h) != GZ_OK) return GZ_E_ARG;   // (before any device call)
  if (c->pending.busy()) { c->err = "gz_heatmap_device while a Compare or phase-B work of the context is in flight"; return GZ_E_STATE; }
  if (!c->have_map_plane) { c->err = "the last comparison stored no distance map"; return GZ_E_STATE; }
  DeviceScope ds_(c);
  if (const int rc = check_tensor_memory(c->device, tensor_view(out, c->w, c->h), "data", &c->err)) return rc;
  TRY(emit_heat(c, heat));
  if (out->consumer_stream) return GZ_OK;   // (ordered on the device: nothing to wait for here)
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GZ_OK;
}

namespace {
// A float plane without a context -> heat.out.  The plane is the caller's device memory (device_plane, `pitch` floats
// per row), or host floats uploaded to a plane from the pool (host_plane, w per row).  The temporaries -- that plane,
// the tables, an event, a stream -- are held as a context-free decode holds its own (DecodeScratch), all or none, and
// go back to the pools when the call has waited for its work.
int heat_of_plane(int device, const float* device_plane, const float* host_plane, int w, int h, int pitch, const HeatRequest& heat) {
  const gz_device_output* out = heat.out;
  if (probe_device(device) != GZ_OK) return GZ_E_NO_DEVICE;
  if (check_tensor_memory(device, tensor_view(out, w, h), "data", nullptr) != GZ_OK) return GZ_E_ARG;
  if (device_plane && check_device_range(device, device_plane, (uint64_t)(h - 1) * (uint64_t)pitch + (uint64_t)(w - 1), sizeof(float), "map", nullptr) != GZ_OK)
    return GZ_E_ARG;
  if (!heat_thresholds().ok) return GZ_E_STATE;
  float* uploaded = nullptr;   // (entered into the scratch's record: declared first, it outlives it)
  DecodeScratch s;
  gz_ctx* c = &s.t;
  c->device = device;
  if (host_plane) {
    TRY(regrow(c, nullptr, nullptr, 0, {{(void**)&s.d_lut, kHeatTabBytes}, {(void**)&uploaded, sizeof(float) * (size_t)w * h}}));
  } else {
    TRY(regrow(c, nullptr, nullptr, 0, {{(void**)&s.d_lut, kHeatTabBytes}}));
  }
  hipStream_t stream = nullptr;
  TRY(s.open_streams(&stream));
  // (a plane of the caller's is complete where the destination is free: on this stream)
  TRY(outputs_after_consumers(c, stream, &s.ev, {out->consumer_stream}));
  HIPCHK(c, upload_heat_tab(s.d_lut, stream));
  if (host_plane) HIPCHK(c, hipMemcpyAsync(uploaded, host_plane, sizeof(float) * (size_t)w * h, hipMemcpyHostToDevice, stream));
  launch_heat(stream, host_plane ? uploaded : device_plane, w, h, pitch, heat, s.d_lut);
  KCHK(c);
  TRY(consumers_after_outputs(c, stream, s.ev, {out->consumer_stream}));
  HIPCHK(c, hipStreamSynchronize(stream));   // (the temporaries go back to the pool behind this)
  s.idle = true;
  return GZ_OK;
}

int heat_of_plane_entry(int device, const float* device_plane, const float* host_plane, int w, int h, int pitch, const HeatRequest& heat) {
  if ((!device_plane && !host_plane) || check_heat_request(heat, w, h) != GZ_OK || pitch < w) return GZ_E_ARG;   // (before any device call)
  CallerDevice keep(device);
  return heat_of_plane(device, device_plane, host_plane, w, h, pitch, heat);
}
}  // namespace

int gz_heatmap_from_map_device(int device, const float* map, int w, int h, int pitch, double good, double bad, const gz_device_output* out) {
  return heat_of_plane_entry(device, map, nullptr, w, h, pitch, HeatRequest{out, good, bad});
}

#ifndef GZ_NO_PROBES
int gz_probe_emit_heat(int device, const float* host_plane, int w, int h, double good, double bad, const gz_device_output* out) {
  return heat_of_plane_entry(device, nullptr, host_plane, w, h, w, HeatRequest{out, good, bad});
}

int gz_probe_heat_thresholds(double* thr255) {
  if (!thr255) return GZ_E_ARG;
  const HeatThresholds& t = heat_thresholds();
  if (!t.ok) return GZ_E_STATE;
  memcpy(thr255, t.thr, sizeof(t.thr));
  return GZ_OK;
}
#endif  // GZ_NO_PROBES

}  // extern "C"
