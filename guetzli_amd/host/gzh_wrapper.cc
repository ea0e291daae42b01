// The C wrapper of the host driver (ctypes: guetzli_amd/encoder.py) and the test hooks of its pieces.
#include <string.h>

#include <algorithm>
#include <exception>

#include "../../include/guetzli_amd.h"
#include "jpeg_reader.h"
#include "jpeg_writer.h"
#include "parallel.h"
#include "png_reader.h"
#include "processor.h"
#include "reader_dump.h"
#include "silver_screen.h"

extern "C" {

// Every entry point below catches what the C++ underneath may throw (std::bad_alloc on a huge
// declared image, ...): nothing propagates through the C boundary.  Return values: >= 0 the
// size of the result (copied only if it fits the caller's buffer: a larger size asks for a
// retry with that much room), -1 failure (message on stderr), -2 exception.
#define GZH_GUARD_BEGIN try {
#define GZH_GUARD_END                                                        \
  } catch (const std::exception& e) {                                        \
    fprintf(stderr, "guetzli_amd: %s\n", e.what());                          \
    return -2;                                                               \
  } catch (...) {                                                            \
    fprintf(stderr, "guetzli_amd: unknown exception\n");                     \
    return -2;                                                               \
  }

static void CopyText(const std::string& s, char* dst, long cap) {
  if (!dst || cap <= 0) return;
  const size_t n = std::min<size_t>(s.size(), (size_t)cap - 1);
  memcpy(dst, s.data(), n);
  dst[n] = 0;
}

static guetzli_amd::Params ParamsFrom(double quality, float target, const int* iparams) {
  guetzli_amd::Params params;
  params.butteraugli_target =
      quality >= 0 ? (float)guetzli_amd::ButteraugliScoreForQuality(quality) : target;
  params.device = iparams[0];
  params.clear_metadata = iparams[1] != 0;
  params.try_420 = iparams[2] != 0;
  params.force_420 = iparams[3] != 0;
  params.use_silver_screen = iparams[4] != 0;
  params.zeroing_greedy_lookahead = iparams[5];
  params.new_zeroing_model = iparams[6] != 0;
  return params;
}

// What a finished Process hands back: the JPEG if it fits, the trace, the timers and counters as "k=v;#k=n;".
static long Deliver(const std::string& jpg, const std::string& dbg, const guetzli_amd::ProcessStats& stats,
                    uint8_t* out, long cap, char* trace, long trace_cap, char* timers, long timers_cap) {
  if ((long)jpg.size() <= cap) memcpy(out, jpg.data(), jpg.size());
  CopyText(dbg, trace, trace_cap);
  if (timers && timers_cap > 0) {
    std::string t;
    for (const auto& kv : stats.timers) {
      char buf[128];
      snprintf(buf, sizeof(buf), "%s=%.6f;", kv.first.c_str(), kv.second);
      t += buf;
    }
    for (const auto& kv : stats.counters) {
      char buf[128];
      snprintf(buf, sizeof(buf), "#%s=%d;", kv.first.c_str(), kv.second);
      t += buf;
    }
    CopyText(t, timers, timers_cap);
  }
  return (long)jpg.size();
}

// guetzli::Process with every field of Params.  jpeg_len < 0: `data` is packed RGB of w x h,
// otherwise JPEG bytes.  quality < 0: `target` is the butteraugli target directly.
// iparams: device, clear_metadata, try_420, force_420, use_silver_screen,
// zeroing_greedy_lookahead, new_zeroing_model.
long gzh_process_params(const uint8_t* data, long jpeg_len, int w, int h, double quality,
                        float target, const int* iparams, uint8_t* out, long cap, char* trace,
                        long trace_cap, char* timers, long timers_cap) {
  GZH_GUARD_BEGIN
  const guetzli_amd::Params params = ParamsFrom(quality, target, iparams);
  guetzli_amd::ProcessStats stats;
  std::string dbg;
  if (trace) stats.debug_output = &dbg;
  std::string jpg;
  bool ok;
  if (jpeg_len < 0) {
    static thread_local std::vector<uint8_t> v;   // Process takes a vector, as the reference's does
    v.assign(data, data + (size_t)3 * w * h);
    ok = guetzli_amd::Process(params, &stats, v, w, h, &jpg);
  } else {
    std::string in((const char*)data, (size_t)jpeg_len);
    ok = guetzli_amd::Process(params, &stats, in, &jpg);
  }
  if (!ok) return -1;
  return Deliver(jpg, dbg, stats, out, cap, trace, trace_cap, timers, timers_cap);
  GZH_GUARD_END
}

// Process(params, stats, DeviceImage, w, h, &out): `image` is a gz_device_pixels (include/guetzli_amd.h) on GPU
// iparams[0]; the other arguments as gzh_process_params'.
long gzh_process_device_pixels(const gz_device_pixels* image, int w, int h, double quality, float target,
                               const int* iparams, uint8_t* out, long cap, char* trace, long trace_cap,
                               char* timers, long timers_cap) {
  GZH_GUARD_BEGIN
  if (!image || image->struct_size != (int)sizeof(gz_device_pixels)) {
    fprintf(stderr, "guetzli_amd: gzh_process_device_pixels: not a gz_device_pixels of this library\n");
    return -1;
  }
  const guetzli_amd::Params params = ParamsFrom(quality, target, iparams);
  guetzli_amd::DeviceImage im;
  im.dtype = image->dtype;
  im.data = image->data;
  im.stride_y = image->stride_y; im.stride_x = image->stride_x; im.stride_c = image->stride_c;
  im.producer_stream = image->producer_stream;
  im.alpha = image->alpha;
  memcpy(im.background, image->background, 3);
  guetzli_amd::ProcessStats stats;
  std::string dbg;
  if (trace) stats.debug_output = &dbg;
  std::string jpg;
  if (!guetzli_amd::Process(params, &stats, im, w, h, &jpg)) return -1;
  return Deliver(jpg, dbg, stats, out, cap, trace, trace_cap, timers, timers_cap);
  GZH_GUARD_END
}

// The same for a gz_device_image: opaque pixels.
long gzh_process_device(const gz_device_image* image, int w, int h, double quality, float target,
                        const int* iparams, uint8_t* out, long cap, char* trace, long trace_cap,
                        char* timers, long timers_cap) {
  if (!image || image->struct_size != (int)sizeof(gz_device_image)) {
    fprintf(stderr, "guetzli_amd: gzh_process_device: not a gz_device_image of this library\n");
    return -1;
  }
  gz_device_pixels px;
  memset(&px, 0, sizeof(px));
  px.struct_size = (int)sizeof(px);
  px.dtype = image->dtype;
  px.data = image->data;
  px.stride_y = image->stride_y; px.stride_x = image->stride_x; px.stride_c = image->stride_c;
  px.producer_stream = image->producer_stream;
  return gzh_process_device_pixels(&px, w, h, quality, target, iparams, out, cap, trace, trace_cap, timers, timers_cap);
}

long gzh_process(const uint8_t* rgb, int w, int h, double quality, float target, int device,
                 uint8_t* out, long cap, char* trace, long trace_cap, char* timers,
                 long timers_cap) {
  const int ip[7] = {device, 1, 0, 0, 0, 3, 1};
  return gzh_process_params(rgb, -1, w, h, quality, target, ip, out, cap, trace, trace_cap, timers,
                            timers_cap);
}

// Process(params, stats, jpeg_data, &out); clear_metadata as Params::clear_metadata.
long gzh_process_jpeg(const uint8_t* data, long len, double quality, float target, int device,
                      int clear_metadata, uint8_t* out, long cap, char* trace, long trace_cap) {
  const int ip[7] = {device, clear_metadata, 0, 0, 0, 3, 1};
  return gzh_process_params(data, len, 0, 0, quality, target, ip, out, cap, trace, trace_cap, nullptr, 0);
}

// The size of a JPEG the reader accepts: wh[0..1] = width, height.  0, or -1 if the stream is rejected.
long gzh_jpeg_size(const uint8_t* data, long len, int* wh) {
  GZH_GUARD_BEGIN
  if (!data || len < 0 || !wh) return -1;
  return guetzli_amd::JpegSize(std::string((const char*)data, (size_t)len), &wh[0], &wh[1]) ? 0 : -1;
  GZH_GUARD_END
}

// DecodeJpegToRGB into `out`, a gz_device_output (include/guetzli_amd.h) on GPU `device` that describes the JPEG's
// w x h pixels (gzh_jpeg_size).  0, or -1 (message on stderr).
// ... and _sized: the stream must hold w x h pixels (a destination sized from the frame header alone), else -1.
long gzh_decode_jpeg_device_sized(const uint8_t* data, long len, int device, const gz_device_output* out, int w, int h) {
  GZH_GUARD_BEGIN
  if (!data || len < 0 || w < 0 || h < 0) return -1;
  if (!out || out->struct_size != (int)sizeof(gz_device_output)) {
    fprintf(stderr, "guetzli_amd: gzh_decode_jpeg_device: not a gz_device_output of this library\n");
    return -1;
  }
  guetzli_amd::DeviceOutput o;
  o.dtype = out->dtype;
  o.data = out->data;
  o.stride_y = out->stride_y; o.stride_x = out->stride_x; o.stride_c = out->stride_c;
  o.consumer_stream = out->consumer_stream;
  return guetzli_amd::DecodeJpegToRGB(std::string((const char*)data, (size_t)len), device, o, nullptr, nullptr, w, h) ? 0 : -1;
  GZH_GUARD_END
}
long gzh_decode_jpeg_device(const uint8_t* data, long len, int device, const gz_device_output* out) {
  return gzh_decode_jpeg_device_sized(data, len, device, out, 0, 0);
}

// DecodeJpegToRGB into packed host bytes: returns 3 * w * h (copied only if it fits `cap`: a larger size asks for a
// retry with that much room -- the frame header says how much, gzh_jpeg_size), -1 on failure.
long gzh_decode_jpeg(const uint8_t* data, long len, int device, uint8_t* host_rgb_out, long cap) {
  GZH_GUARD_BEGIN
  if (!data || len < 0) return -1;
  std::vector<uint8_t> rgb;
  int w = 0, h = 0;
  if (!guetzli_amd::DecodeJpegToRGB(std::string((const char*)data, (size_t)len), device, &rgb, &w, &h)) return -1;
  if (host_rgb_out && (long)rgb.size() <= cap) memcpy(host_rgb_out, rgb.data(), rgb.size());
  return (long)rgb.size();
  GZH_GUARD_END
}

// What a decode says of its entropy path: info[0] 1 = the device's coefficients were used, 0 = the host's; info[1] the
// gz_scan_result status of the attempt, -1 = none; info[2] subsequences; info[3] inter-workgroup rounds; info[4] end_offset;
// info[5] what gz_decode_scan* returned (0, or the GZ_E_* code of a call that failed and fell back).
static void CopyDecodeInfo(const guetzli_amd::DecodeInfo& di, int64_t* info) {
  if (!info) return;
  info[0] = di.device_path ? 1 : 0;
  info[1] = di.status;
  info[2] = di.subsequences;
  info[3] = di.sync_rounds;
  info[4] = (int64_t)di.end_offset;
  info[5] = di.rc;
}
static guetzli_amd::EntropyOptions EntropyFrom(const int* mode) {   // mode: device (0 / 1), subseq_bytes, max_sync_rounds
  guetzli_amd::EntropyOptions e;
  if (mode) {
    e.device = mode[0] != 0;
    e.subseq_bytes = mode[1];
    e.max_sync_rounds = mode[2];
  }
  return e;
}

// gzh_decode_jpeg_device_sized with the entropy path chosen by mode[3] (EntropyFrom; NULL: the host) and reported in
// info[6] (CopyDecodeInfo; may be NULL).
long gzh_decode_jpeg_device_entropy(const uint8_t* data, long len, int device, const gz_device_output* out, int w, int h,
                                    const int* mode, int64_t* info) {
  GZH_GUARD_BEGIN
  if (!data || len < 0 || w < 0 || h < 0) return -1;
  if (!out || out->struct_size != (int)sizeof(gz_device_output)) {
    fprintf(stderr, "guetzli_amd: gzh_decode_jpeg_device_entropy: not a gz_device_output of this library\n");
    return -1;
  }
  guetzli_amd::DeviceOutput o;
  o.dtype = out->dtype;
  o.data = out->data;
  o.stride_y = out->stride_y; o.stride_x = out->stride_x; o.stride_c = out->stride_c;
  o.consumer_stream = out->consumer_stream;
  guetzli_amd::DecodeInfo di;
  const bool ok = guetzli_amd::DecodeJpegToRGB(std::string((const char*)data, (size_t)len), device, o, nullptr, nullptr, w, h,
                                               EntropyFrom(mode), &di);
  CopyDecodeInfo(di, info);
  return ok ? 0 : -1;
  GZH_GUARD_END
}

// DecodeJpegBatchToRGB: the n JPEGs data[i] (lens[i] bytes) of w x h pixels each into the n images of `out`, a
// gz_device_output_batch (include/guetzli_amd.h) on GPU `device`; mode as above, scratch_bytes = the device call's
// scratch_cap_bytes; info[6 n] (CopyDecodeInfo per image; may be NULL).  0, or -1 (message on stderr) with *failed (may be
// NULL) the index of the file that was refused, -1 where the arguments were.
long gzh_decode_jpeg_batch_device(const uint8_t* const* data, const long* lens, int n, int device, const gz_device_output_batch* out, int w,
                                  int h, const int* mode, uint64_t scratch_bytes, int64_t* info, int* failed) {
  GZH_GUARD_BEGIN
  if (failed) *failed = -1;
  if (!data || !lens || n < 1 || w < 0 || h < 0) return -1;
  if (!out || out->struct_size != (int)sizeof(gz_device_output_batch) || out->n != n) {
    fprintf(stderr, "guetzli_amd: gzh_decode_jpeg_batch_device: not a gz_device_output_batch of this library and of n images\n");
    return -1;
  }
  std::vector<std::string> jpegs((size_t)n);
  for (int i = 0; i < n; ++i) {
    if (!data[i] || lens[i] < 0) return -1;
    jpegs[(size_t)i].assign((const char*)data[i], (size_t)lens[i]);
  }
  guetzli_amd::DeviceOutputBatch o;
  o.dtype = out->dtype;
  o.data = out->data;
  o.stride_n = out->stride_n; o.stride_y = out->stride_y; o.stride_x = out->stride_x; o.stride_c = out->stride_c;
  o.consumer_stream = out->consumer_stream;
  std::vector<guetzli_amd::DecodeInfo> infos;
  const bool ok = guetzli_amd::DecodeJpegBatchToRGB(jpegs, device, o, w, h, EntropyFrom(mode), &infos, failed, (size_t)scratch_bytes);
  if (info)
    for (size_t i = 0; i < infos.size(); ++i) CopyDecodeInfo(infos[i], info + 6 * i);
  return ok ? 0 : -1;
  GZH_GUARD_END
}

// The stream's dequantised coefficients in the frame layout (what DecodeJpegToRGB hands to the device) by either entropy
// path: returns their count (copied if it fits `cap` elements), -1 if the stream is refused; whf[3] = width, height,
// chroma factor; info as above.  meta (optional, meta_cap bytes): what the reader kept beside the coefficients -- every
// APPn, COM and the tail, each behind its length as 8 decimal digits -- and *meta_len its size.  Test hook.
long gzh_decode_jpeg_coeffs(const uint8_t* data, long len, int device, const int* mode, int* whf, int16_t* out, long cap,
                            int64_t* info, uint8_t* meta, long meta_cap, long* meta_len) {
  GZH_GUARD_BEGIN
  if (!data || len < 0 || !whf) return -1;
  std::vector<int16_t> coeffs;
  guetzli_amd::DecodeInfo di;
  guetzli_amd::JpegInput jpg;
  const bool ok = guetzli_amd::DecodeJpegCoeffs(std::string((const char*)data, (size_t)len), device, EntropyFrom(mode), &whf[0],
                                                &whf[1], &whf[2], &coeffs, &di, &jpg);
  CopyDecodeInfo(di, info);
  if (!ok) return -1;
  if (out && (long)coeffs.size() <= cap) memcpy(out, coeffs.data(), coeffs.size() * sizeof(int16_t));
  std::string m;
  auto add = [&m](char tag, const std::string& s) {
    char head[16];
    snprintf(head, sizeof(head), "%c%08zu", tag, s.size());
    m += head;
    m += s;
  };
  for (const std::string& s : jpg.app_data) add('A', s);
  for (const std::string& s : jpg.com_data) add('C', s);
  add('T', jpg.tail_data);
  if (meta_len) *meta_len = (long)m.size();
  if (meta && (long)m.size() <= meta_cap) memcpy(meta, m.data(), m.size());
  return (long)coeffs.size();
  GZH_GUARD_END
}

// Process(params, stats, jpeg_data, &out, EntropyOptions, &info): gzh_process_jpeg with every field of Params
// (iparams as gzh_process_params'), the input's entropy path chosen by mode[3] (EntropyFrom; NULL: the host) and
// reported in info[6] (CopyDecodeInfo; may be NULL; written whether the encode succeeds or not).
long gzh_process_jpeg_entropy(const uint8_t* data, long len, double quality, float target, const int* iparams, const int* mode,
                              int64_t* info, uint8_t* out, long cap, char* trace, long trace_cap, char* timers, long timers_cap) {
  GZH_GUARD_BEGIN
  if (!data || len < 0 || !iparams) return -1;
  const guetzli_amd::Params params = ParamsFrom(quality, target, iparams);
  guetzli_amd::ProcessStats stats;
  std::string dbg;
  if (trace) stats.debug_output = &dbg;
  std::string jpg;
  guetzli_amd::DecodeInfo di;
  const bool ok = guetzli_amd::Process(params, &stats, std::string((const char*)data, (size_t)len), &jpg, EntropyFrom(mode), &di);
  CopyDecodeInfo(di, info);
  if (!ok) return -1;
  return Deliver(jpg, dbg, stats, out, cap, trace, trace_cap, timers, timers_cap);
  GZH_GUARD_END
}

double gzh_butteraugli_score_for_quality(double q) {
  return guetzli_amd::ButteraugliScoreForQuality(q);
}

// Length-limited Huffman depths of a 257-entry histogram (CreateHuffmanTree, entropy_encode.cc:
// 73-145), the way phase B's size model calls it (stream: see jpeg_writer.h).  Test hook.
void gzh_huffman_depths(const uint32_t* counts, int tree_limit, uint8_t* depth, int stream) {
  guetzli_amd::HuffmanDepths(counts, (size_t)guetzli_amd::kHistoSize, tree_limit, depth, stream);
}

// Threads of the driver's worker pool (the calling thread included): min(16, cores the process may
// run on), GZ_HOST_THREADS overrides.  Test hook for the per-rank core share of a multi-GPU run.
int gzh_worker_pool_size() { return guetzli_amd::WorkerPool::Get().size(); }

// ReadJpeg as a canonical dump (test hook; the format: reader_dump.h).  Returns the dump size (copied if it
// fits), or -1 if the stream is rejected.
long gzh_read_jpeg(const uint8_t* data, long len, uint8_t* out, long cap) {
  GZH_GUARD_BEGIN
  guetzli_amd::JpegInput jpg;
  std::string err;
  if (!guetzli_amd::ReadJpeg(data, (size_t)len, &jpg, &err)) return -1;
  const std::string d = guetzli_amd::DumpJpegInput(jpg);
  if ((long)d.size() <= cap) memcpy(out, d.data(), d.size());
  return (long)d.size();
  GZH_GUARD_END
}

// The same from the reader as an encode of JPEG input calls it (ReadJpegInput), the scan read as mode[3] says on GPU
// `device`; info[6] as above (may be NULL).  Test hook, the twin of gzh_read_jpeg.
long gzh_read_jpeg_entropy(const uint8_t* data, long len, int device, const int* mode, int64_t* info, uint8_t* out, long cap) {
  GZH_GUARD_BEGIN
  if (!data || len < 0) return -1;
  guetzli_amd::JpegInput jpg;
  guetzli_amd::DecodeInfo di;
  const bool ok = guetzli_amd::ReadJpegInput(std::string((const char*)data, (size_t)len), device, EntropyFrom(mode), &jpg, nullptr, &di);
  CopyDecodeInfo(di, info);
  if (!ok) return -1;
  const std::string d = guetzli_amd::DumpJpegInput(jpg);
  if (out && (long)d.size() <= cap) memcpy(out, d.data(), d.size());
  return (long)d.size();
  GZH_GUARD_END
}

// ReadPNG (guetzli.cc:47-152): PNG bytes -> packed RGB with alpha blended on black.  Returns
// 3*w*h (copied to out if it fits) and the dimensions in wh[0..1], or -1 if the stream is
// rejected (message on stderr).
long gzh_read_png(const uint8_t* data, long len, int* wh, uint8_t* out, long cap) {
  GZH_GUARD_BEGIN
  std::vector<uint8_t> rgb;
  std::string err;
  int w = 0, h = 0;
  if (!guetzli_amd::ReadPng(data, (size_t)len, &w, &h, &rgb, &err)) {
    fprintf(stderr, "Error reading PNG data from input file: %s\n", err.c_str());
    return -1;
  }
  wh[0] = w;
  wh[1] = h;
  if ((long)rgb.size() <= cap) memcpy(out, rgb.data(), rgb.size());
  return (long)rgb.size();
  GZH_GUARD_END
}

// SilverScreenYUV420 (silver_screen.h: RGBToYUV420 on the host, with libm): rgb w*h*3 -> y, u, v of w*h floats each.
// Test hook: the yardstick of the device path (gz_downsample_silver, gz_probe_silver_yuv420).
int gzh_silver_screen_yuv420(const uint8_t* rgb, int w, int h, float* y, float* u, float* v) {
  GZH_GUARD_BEGIN
  if (!rgb || !y || !u || !v || w <= 0 || h <= 0) return -1;
  std::vector<float> py, pu, pv;
  guetzli_amd::SilverScreenYUV420(rgb, w, h, &py, &pu, &pv);
  const size_t n = (size_t)w * h;
  memcpy(y, py.data(), n * sizeof(float));
  memcpy(u, pu.data(), n * sizeof(float));
  memcpy(v, pv.data(), n * sizeof(float));
  return 0;
  GZH_GUARD_END
}

// WriteJpeg of an image given by dequantised coefficients + quant matrices, for a frame with chroma subsampling
// factor 1 or 2 (coefficients in the frame layout of include/guetzli_amd.h).  Test hook.
long gzh_write_jpeg_factor(const int16_t* coeffs, int w, int h, const int* q, int original,
                           int factor, uint8_t* out, long cap) {
  GZH_GUARD_BEGIN
  guetzli_amd::Frame f;
  if (original) {
    guetzli_amd::FrameFromOriginal(coeffs, w, h, &f);
  } else {
    int qq[3][64];
    memcpy(qq, q, sizeof(qq));
    guetzli_amd::FrameFromImageFactor(coeffs, qq, w, h, factor, &f);
  }
  std::string s;
  if (!guetzli_amd::WriteJpeg(f, &s)) return -1;
  if ((long)s.size() <= cap) memcpy(out, s.data(), s.size());
  return (long)s.size();
  GZH_GUARD_END
}

// The same for a 4:4:4 frame.
long gzh_write_jpeg(const int16_t* coeffs, int w, int h, const int* q, int original,
                    uint8_t* out, long cap) {
  return gzh_write_jpeg_factor(coeffs, w, h, q, original, 1, out, cap);
}

// Marker segments + Huffman codes from symbol counts (test hook of BuildJpegHead):
// counts uint32 [2][3][256] as gz_jpeg_histograms returns them; q null = the q=1 original.
// Returns the head length (bytes copied to head_out if they fit) or -1.
long gzh_jpeg_head_factor(const uint32_t* counts, const int* q, int w, int h, int ncomp, int factor,
                          uint8_t* head_out, long cap, uint8_t* depth /*[2][3][256]*/,
                          uint16_t* code /*[2][3][256]*/) {
  GZH_GUARD_BEGIN
  guetzli_amd::SymbolHistogram dc[3], ac[3];
  for (int c = 0; c < 3; ++c)
    for (int i = 0; i < 256; ++i) {
      dc[c].Add(i, (int)counts[(0 * 3 + c) * 256 + i]);
      ac[c].Add(i, (int)counts[(1 * 3 + c) * 256 + i]);
    }
  guetzli_amd::Frame f;
  int qq[3][64];
  if (q) memcpy(qq, q, sizeof(qq));
  guetzli_amd::FrameTablesFactor(q ? qq : nullptr, w, h, ncomp, factor, &f);
  guetzli_amd::JpegHead head;
  if (!guetzli_amd::BuildJpegHead(f, dc, ac, &head)) return -1;
  if ((long)head.bytes.size() <= cap) memcpy(head_out, head.bytes.data(), head.bytes.size());
  memcpy(depth, head.depth, sizeof(head.depth));
  memcpy(code, head.code, sizeof(head.code));
  return (long)head.bytes.size();
  GZH_GUARD_END
}

long gzh_jpeg_head(const uint32_t* counts, const int* q, int w, int h, int ncomp,
                   uint8_t* head_out, long cap, uint8_t* depth /*[2][3][256]*/,
                   uint16_t* code /*[2][3][256]*/) {
  return gzh_jpeg_head_factor(counts, q, w, h, ncomp, 1, head_out, cap, depth, code);
}

}  // extern "C"
