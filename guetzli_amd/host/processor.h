// Host search driver over the C ABI of include/guetzli_amd.h: the drop-in for
// guetzli::Process(params, stats, rgb, w, h, &out) (processor.h:54-56,
// processor.cc:926-948) with all per-pixel / per-block numeric work on the MI355X.
//
// Same names, argument meaning and error behaviour as the reference API: bool return,
// diagnostics on stderr, no exceptions; `ProcessStats::debug_output` receives the same
// --verbose trace text (one line per candidate evaluation), which is what the parity
// tests compare first.
//
// What stays on the host is the serial decision logic of the reference (quant-matrix
// bisection, global coefficient ordering, entropy-size model) and the JPEG writer; it is
// written from scratch around flat coefficient arrays.  Scope: everything guetzli::Process
// accepts -- RGB input (the BASELINE configurations), YUV 4:4:4 and 4:2:0 JPEG input, every
// field of Params (try_420 / force_420 / use_silver_screen included).
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <map>
#include <string>
#include <vector>

namespace guetzli_amd {

struct Params {                       // guetzli::Params, processor.h:29-37
  float butteraugli_target = 1.0;
  bool clear_metadata = true;
  bool try_420 = false;
  bool force_420 = false;
  bool use_silver_screen = false;
  int zeroing_greedy_lookahead = 3;
  bool new_zeroing_model = true;
  int device = 0;                     // HIP device ordinal (not in the reference)
};

static const char* const kNumItersCnt = "number of iterations";
static const char* const kNumItersUpCnt = "number of iterations up";
static const char* const kNumItersDownCnt = "number of iterations down";

struct ProcessStats {                 // guetzli::ProcessStats, stats.h:34-41
  std::map<std::string, int> counters;
  std::string* debug_output = nullptr;
  FILE* debug_output_file = nullptr;
  std::string filename;
  // wall-clock breakdown in seconds, filled by Process (not in the reference)
  std::map<std::string, double> timers;
};

// gz_device_pixels of include/guetzli_amd.h: a w x h x 3 image that already lives in the memory of GPU
// Params::device.  Element (y, x, c) is data[y*stride_y + x*stride_x + c*stride_c], strides in elements, >= 0.
// With alpha != nullptr pixel (y, x) has the alpha sample alpha[y*stride_y + x*stride_x], of the colours' dtype, and
// is blended over `background` as the PNG front end blends over black: (v * a + bg * (255 - a) + 128) / 255 on bytes.
struct DeviceImage {
  enum Dtype { kU8 = 0, kF32 = 1, kF16 = 2, kBF16 = 3, kU16 = 4 };   // GZ_DT_* (kU16: the high byte counts)
  int dtype = kU8;
  const void* data = nullptr;         // device address of element (0, 0, 0)
  int64_t stride_y = 0, stride_x = 0, stride_c = 0;
  void* producer_stream = nullptr;    // hipStream_t whose work writes the data; nullptr: none to wait for
  const void* alpha = nullptr;        // device address of the alpha sample of pixel (0, 0); nullptr: opaque
  uint8_t background[3] = {0, 0, 0};  // r, g, b
};

// gz_device_output of include/guetzli_amd.h: where decoded pixels go, a w x h x 3 image in the memory of GPU `device`.
// Element (y, x, c) is data[y*stride_y + x*stride_x + c*stride_c], strides in elements; no two elements may share an
// address.  A byte b arrives as b (kU8), b * 257 (kU16) or b / 255 (the three float types).
struct DeviceOutput {
  int dtype = DeviceImage::kU8;       // DeviceImage::Dtype
  void* data = nullptr;               // device address of element (0, 0, 0)
  int64_t stride_y = 0, stride_x = 0, stride_c = 0;
  void* consumer_stream = nullptr;    // hipStream_t that used the memory before and reads it after; nullptr: none
};

double ButteraugliScoreForQuality(double quality);                       // quality.cc:78-85
double ScoreJPEG(double butteraugli_distance, int size, double target);  // score.cc:23-41

// Sets *out to a JPEG that decodes to an image visually indistinguishable from rgb
// (packed 8-bit sRGB, w*h*3).  Returns false (message on stderr) on failure.
bool Process(const Params& params, ProcessStats* stats, const std::vector<uint8_t>& rgb,
             int w, int h, std::string* out);

// The same from pixels on the GPU (floats: [0, 1] -> rint(x * 255), clamped; uint16: the high byte; alpha blended over
// the background; include/guetzli_amd.h has the rules):
// nothing goes through host memory but, for w or h < 32, the bytes of the tiny image itself.  Same refusals and
// messages as above; memory that GPU params.device cannot read is a failure, not a fault.
bool Process(const Params& params, ProcessStats* stats, const DeviceImage& image, int w, int h,
             std::string* out);

// The same from an existing JPEG (guetzli::Process(params, stats, jpeg_data, &out),
// processor.h:39-41): the input is parsed on the host (jpeg_reader.h), its coefficients become
// the original, its decoded pixels the comparator's reference image, its quantisation the
// first candidate; Params::clear_metadata decides whether APPn / COM / trailing bytes are
// carried over.  YUV 4:4:4 and 4:2:0 input (other sampling factors are refused, as the reference
// refuses them, processor.cc:811-823).
bool Process(const Params& params, ProcessStats* stats, const std::string& jpeg_data,
             std::string* out);

// guetzli::DecodeJpegToRGB (jpeg_data_decoder.cc:45-54) with the pixels left on the GPU: the stream is read on the host
// (jpeg_reader.h), its coefficients are dequantised, and the device computes OutputImage::ToSRGB of them -- the pixel
// model every butteraugli distance of a search is computed on -- into `out`.  Accepts what the reference's function
// returns pixels for: one component (grey: the two chroma components are zero), or three with a YCbCr colour space in
// 4:4:4 or 4:2:0; everything else is refused with a message on stderr and false.  *w, *h (either may be null) receive
// the image's size -- `out` must describe that many pixels: JpegSize tells beforehand, and a caller that has sized
// `out` some other way says for which size (expect_w, expect_h > 0): a stream of another size is refused, not written.
bool DecodeJpegToRGB(const std::string& jpeg, int device, const DeviceOutput& out, int* w, int* h, int expect_w = 0,
                     int expect_h = 0);
// The same into packed host bytes, rgb[(y * w + x) * 3 + c].
bool DecodeJpegToRGB(const std::string& jpeg, int device, std::vector<uint8_t>* rgb, int* w, int* h);

// Who reads the entropy-coded scan.  device: an eligible scan (jpeg_reader.h: ScanRequest) is read by the device's
// self-synchronising Huffman decoder (gz_decode_scan*), and only the stream's bytes go up instead of its coefficients;
// every other scan, and every scan the device hands back (a status other than GZ_SCAN_DECODED, any error of the call), is
// read by the host as if nothing had been tried.  Which streams are accepted, and what they decode to, does not
// depend on it.  One difference: with a DeviceOutput, a stream that the reader refuses BEHIND a scan the device decoded
// (garbage where a marker should be, an Adobe marker after the scan that makes the colour space RGB) is refused as always,
// but the destination may have been written by then.
struct EntropyOptions {
  bool device = false;
  int subseq_bytes = 0, max_sync_rounds = 0;   // gz_scan's; 0 = the library's defaults
};
struct DecodeInfo {
  bool device_path = false;    // the device's coefficients were used
  int status = -1;             // gz_scan_result's of the attempt; -1: no verdict (host asked for, no eligible scan, or rc != 0)
  int rc = 0;                  // what gz_decode_scan* returned (GZ_OK, GZ_E_HIP, GZ_E_NOMEM ...): a failed call falls back too
  int subsequences = 0, sync_rounds = 0;
  uint64_t end_offset = 0;
};
bool DecodeJpegToRGB(const std::string& jpeg, int device, const DeviceOutput& out, int* w, int* h, int expect_w, int expect_h,
                     const EntropyOptions& entropy, DecodeInfo* info = nullptr);
bool DecodeJpegToRGB(const std::string& jpeg, int device, std::vector<uint8_t>* rgb, int* w, int* h, const EntropyOptions& entropy,
                     DecodeInfo* info = nullptr);
// N JPEGs of ONE decoded size into the N images of a strided tensor on GPU `device` (gz_device_output_batch: element
// (i, y, x, c) at data[i*stride_n + y*stride_y + x*stride_x + c*stride_c], no two elements at one address): image i is,
// bit for bit, what DecodeJpegToRGB(jpegs[i], ...) writes, and (*infos)[i] what it reports.  With entropy.device the
// eligible scans of the whole batch are read by ONE device call per sampling (gz_decode_scan_batch_device: grey, 4:4:4,
// 4:2:0 -- three at the most): every file is parsed up to its scan, the device decodes, and every file is parsed again
// with the verdict in hand, so that whatever follows the scan is judged as ever.  A file whose scan is not eligible, or
// got a status other than DECODED, or whose device call failed (one line on stderr), is read by the host into its image,
// silently.  expect_w, expect_h: the size `out` was made for (0: the first file's).  A file the reader refuses, or of
// another size, fails the call -- *failed (optional) is its index -- and `out` then holds no guarantee.
// scratch_cap_bytes: gz_decode_scan_batch_device's.
struct DeviceOutputBatch {
  int dtype = DeviceImage::kU8;
  void* data = nullptr;
  int64_t stride_n = 0, stride_y = 0, stride_x = 0, stride_c = 0;
  void* consumer_stream = nullptr;
};
bool DecodeJpegBatchToRGB(const std::vector<std::string>& jpegs, int device, const DeviceOutputBatch& out, int expect_w, int expect_h,
                          const EntropyOptions& entropy, std::vector<DecodeInfo>* infos = nullptr, int* failed = nullptr,
                          size_t scratch_cap_bytes = 0);
// The stream's dequantised coefficients in the frame layout of include/guetzli_amd.h (what DecodeJpegToRGB hands to the
// device), *factor the chroma subsampling factor; meta (optional) receives what the reader kept beside them.
struct JpegInput;
bool DecodeJpegCoeffs(const std::string& jpeg, int device, const EntropyOptions& entropy, int* w, int* h, int* factor,
                      std::vector<int16_t>* coeffs, DecodeInfo* info = nullptr, JpegInput* meta = nullptr);
// Process(params, stats, jpeg_data, &out) with the input's scan read as `entropy` says.  device: an eligible scan --
// grey, 4:4:4 or 4:2:0, whatever its colour space -- is read by the device's decoder in its input mode
// (gz_decode_scan_input: the READER's result, quantised values on the grids padded to whole MCUs), and CheckJpegSanity's
// verdict comes from the device too; any other scan, any status other than GZ_SCAN_DECODED and any failing call (one
// line on stderr) leave the scan to the host's block loop, silently.  Verdict, messages, output bytes and trace do not
// depend on it; *info (optional) says which path the input took.  The overload above is this one with EntropyOptions().
bool Process(const Params& params, ProcessStats* stats, const std::string& jpeg_data, std::string* out,
             const EntropyOptions& entropy, DecodeInfo* info = nullptr);
// ReadJpeg as that encode calls it: *jpg as the host's block loop leaves it by either path (`coeffs` of every component
// filled, scan_decoded_elsewhere false); *large_coeff (optional): CheckJpegSanity's verdict where the device path ran
// (info->device_path), false otherwise -- the caller then runs the check itself.
bool ReadJpegInput(const std::string& jpeg, int device, const EntropyOptions& entropy, JpegInput* jpg, bool* large_coeff = nullptr,
                   DecodeInfo* info = nullptr);
// The size the frame header declares (of a stream ReadJpeg accepts).
bool JpegSize(const std::string& jpeg, int* w, int* h);

}  // namespace guetzli_amd
