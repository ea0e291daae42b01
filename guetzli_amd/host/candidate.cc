// One candidate of the search: its symbol statistics from the device, its JPEG (head on the host, scan on
// the device), its comparison and whether it becomes the output -- and the quant-matrix trials built on them.
#include <string.h>

#include "encoder.h"

namespace guetzli_amd {

void Encoder::Tables(const int (*q)[64], int ncomp, Frame* f) const {
  FrameTablesFactor(q, w_, h_, ncomp, fac_, f);
  if (!jpeg_input_) return;
  f->meta = &meta_;
  if (q == nullptr) InputTables(f);
}

void Encoder::InputTables(Frame* f) const {
  f->quant = in_quant_;
  for (int c = 0; c < 3; ++c) {
    f->quant_idx[c] = in_quant_idx_[c];
    f->comp_id[c] = in_comp_id_[c];
  }
}

// BuildDCHistograms + BuildACHistograms of the frame SaveToJpegData would write.  In a 4:2:0
// frame the luma statistics depend on whether chroma is written at all (MCU order and padding
// blocks, or luma alone in raster order): asked for three components first, and again for one
// if both chroma components turn out to be all zero.
bool Encoder::DeviceHistograms(const QuantMatrix q, SymbolHistogram* dc, SymbolHistogram* ac, int ncomp) {
  std::vector<uint32_t> counts(2 * 3 * 256);
  const int rc = gz_jpeg_histograms_ncomp(ctx_, &q[0][0], ncomp, counts.data());
  if (rc != GZ_OK) return Fail("gz_jpeg_histograms", rc);
  for (int c = 0; c < 3; ++c) {
    dc[c].Clear();
    ac[c].Clear();
    for (int i = 0; i < 256; ++i) {
      dc[c].Add(i, (int)counts[(0 * 3 + c) * 256 + i]);
      ac[c].Add(i, (int)counts[(1 * 3 + c) * 256 + i]);
    }
  }
  if (ncomp == 3 && fac_ == 2 && ChromaAllZero(dc, ac)) return DeviceHistograms(q, dc, ac, 1);
  return true;
}

// Serialize in two halves.  PrepareHead + ScanBegin: the marker segments and Huffman codes on the host, then
// the scan enqueued on the context's entropy stream (gz_jpeg_scan_begin) -- the caller goes on
// enqueueing (the next order's construction) while the entropy coder runs beside the
// evaluation.  SerializeEnd collects the scan's length.
bool Encoder::Serialize(const int (*q)[64], const SymbolHistogram* dc, const SymbolHistogram* ac,
                        size_t* size) {
  return PrepareHead(q, dc, ac) && ScanBegin() && SerializeEnd(q, size);
}

// The host's half of a candidate's JPEG: marker segments and Huffman codes (head_), and -- from the
// same symbol statistics -- the exact number of bits of its scan: every symbol occurrence costs its
// code length plus its extra bits (the low nibble of an AC symbol, the category of a DC symbol:
// jpeg_data_writer.cc:446-497), so the scan is head_bits_ long before a single bit is written.
bool Encoder::PrepareHead(const int (*q)[64], const SymbolHistogram* dc, const SymbolHistogram* ac) {
  Stopwatch sw;
  Frame f;
  // a single component is written when both chroma planes are entirely zero
  // (OutputImage::SaveToJpegData, output_image.cc:348-409); the q=1 original always has 3
  const int nc = q && ChromaAllZero(dc, ac) ? 1 : 3;
  Tables(q, nc, &f);
  SymbolHistogram dc1[3], ac1[3];
  if (nc == 1 && fac_ == 2) {
    // luma alone is written in raster order without padding blocks: its statistics are not
    // those of the 4:2:0 MCU order the caller may hold (chroma that became all zero during
    // the search); recounted
    if (!DeviceHistograms(q, dc1, ac1, 1)) return false;
    dc = dc1;
    ac = ac1;
  }
  if (!BuildJpegHead(f, dc, ac, &head_)) return Fail("BuildJpegHead", GZ_E_STATE);
  head_bits_ = 0;
  for (int c = 0; c < head_.ncomp; ++c)
    head_bits_ += (uint64_t)HistogramRawBits(dc[c], head_.depth[0][c]) +
                  (uint64_t)HistogramRawBits(ac[c], head_.depth[1][c]);
  { const double d = sw.lap(); timer_[kTWrite] += d; timer_[kTHead] += d; }
  return true;
}

bool Encoder::ScanBegin() {
  Stopwatch sw;
  const int rc = gz_jpeg_scan_begin(ctx_, head_.ncomp, &head_.depth[0][0][0], &head_.code[0][0][0]);
  { const double d = sw.lap(); timer_[kTWrite] += d; timer_[kTScanBegin] += d; }
  if (rc != GZ_OK) return Fail("gz_jpeg_scan", rc);
  return true;
}

// What the candidate's JPEG weighs at least: its head, its scan's bits as bytes -- the 0x00 stuffed
// behind every 0xFF byte of the scan (jpeg_bit_writer.h:62-70) only adds to that -- and EOI.
size_t Encoder::SizeLowerBound() const {
  size_t size = head_.bytes.size() + (size_t)((head_bits_ + 7) / 8) + 2;
  if (jpeg_input_ && !meta_.strip) size += meta_.tail_data.size();
  return size;
}
bool Encoder::SerializeEnd(const int (*q)[64], size_t* size) {
  Stopwatch sw;
  uint64_t scan_bytes = 0;
  const int rc = gz_jpeg_scan_end(ctx_, &scan_bytes);
  if (rc != GZ_OK) return Fail("gz_jpeg_scan", rc);
  *size = head_.bytes.size() + (size_t)scan_bytes + 2;   // + EOI
  if (jpeg_input_ && !meta_.strip) *size += meta_.tail_data.size();
  { const double d = sw.lap(); timer_[kTWrite] += d; timer_[kTScanEnd] += d; }
  ++count_[kNScans];
  if (!knobs_.verify()) return true;
  // GZ_VERIFY_ENTROPY: the bit count derived from the statistics is the coder's
  uint64_t bits = 0, ff = 0;
  const int rb = gz_jpeg_scan_bits(ctx_, &bits, &ff);
  if (rb != GZ_OK) return Fail("gz_jpeg_scan_bits", rb);
  if (bits != head_bits_ || (bits + 7) / 8 + ff != scan_bytes || SizeLowerBound() > *size) {
    fprintf(stderr, "guetzli_amd: scan of %llu bits (+%llu stuffed bytes), the symbol statistics say %llu\n",
            (unsigned long long)bits, (unsigned long long)ff, (unsigned long long)head_bits_);
    return false;
  }
  return VerifyAgainstHostWriter(q, *size);
}

// Test hook (GZ_VERIFY_ENTROPY=1): the device scan + host head must equal the serial host
// writer on the same coefficients, byte for byte.
bool Encoder::VerifyAgainstHostWriter(const int (*q)[64], size_t size) {
  std::vector<int16_t> co((size_t)nblk_ * 64);
  int rc = gz_get_coeffs(ctx_, co.data());
  if (rc != GZ_OK) return Fail("gz_get_coeffs", rc);
  const std::vector<int16_t>& img = sc_.img;
  if (q && mirror_valid_ && memcmp(co.data(), img.data(), co.size() * 2) != 0) {
    size_t nd = 0, first = 0;
    for (size_t i = 0; i < co.size(); ++i)
      if (co[i] != img[i]) { if (!nd) first = i; ++nd; }
    fprintf(stderr, "guetzli_amd: host mirror of the image differs from the device image "
            "(%zu coefficients, first at %zu: device %d host %d)\n", nd, first, co[first], img[first]);
    return false;
  }
  Frame f;
  if (q) {
    FrameFromImageFactor(co.data(), q, w_, h_, fac_, &f);
  } else if (jpeg_input_) {   // the input as read: quantised by its own tables
    FrameFromImageFactor(co.data(), q_in_, w_, h_, fac_, &f);
    if (f.ncomp != 3) return true;   // (all-zero chroma in the input: not comparable this way)
    InputTables(&f);
  } else {
    FrameFromOriginal(co.data(), w_, h_, &f);
  }
  if (jpeg_input_) f.meta = &meta_;
  std::string ref;
  WriteJpeg(f, &ref);
  std::string got = head_.bytes;
  std::vector<uint8_t> scan(3 * co.size() + 1024);
  size_t n = 0;
  rc = gz_jpeg_scan_bytes(ctx_, 0, scan.data(), scan.size(), &n);
  if (rc != GZ_OK) return Fail("gz_jpeg_scan_bytes", rc);
  got.append((const char*)scan.data(), n);
  got.push_back((char)0xff);
  got.push_back((char)0xd9);
  if (jpeg_input_ && !meta_.strip) got.append(meta_.tail_data);
  if (got != ref || got.size() != size) {
    fprintf(stderr, "guetzli_amd: device entropy coder mismatch (device %zu/%zu bytes, host %zu)\n",
            got.size(), size, ref.size());
    return false;
  }
  return true;
}

// comparator_->Compare(*img) in two halves: the evaluation is enqueued before the candidate's
// Huffman codes are built on the host (Serialize) and collected afterwards.
bool Encoder::CompareBegin() {
  Stopwatch sw;
  const int rc = gz_compare_begin(ctx_);
  { const double d = sw.lap(); timer_[kTCompare] += d; timer_[kTCmpBegin] += d; }
  if (rc != GZ_OK) return Fail("gz_compare_begin", rc);
  return true;
}
bool Encoder::CompareCurrent() {
  Stopwatch sw;
  const int rc = gz_compare_end(ctx_, &distance_);
  { const double d = sw.lap(); timer_[kTCompare] += d; timer_[kTCmpEnd] += d; }
  if (rc != GZ_OK) return Fail("gz_compare_end", rc);
  Log(" BA[100.00%%] D[%6.4f]", distance_);
  return true;
}

bool Encoder::MaybeOutput(size_t size) {   // processor.cc:139-148
  const double score = ScoreJPEG(distance_, (int)size, params_.butteraugli_target);
  Log(" Score[%.4f]", score);
  if (score < best_score_ || best_score_ < 0) {
    best_head_ = head_.bytes;
    const int rc = gz_jpeg_scan_keep(ctx_);
    if (rc != GZ_OK) return Fail("gz_jpeg_scan_keep", rc);
    best_score_ = score;
    best_size_ = size;
    best_on_host_ = false;
    Log(" (*)");
  }
  Log("\n");
  return true;
}

// img := orig, then ApplyGlobalQuantization(q); device and host copies.
bool Encoder::SetImageFromQuantization(const QuantMatrix q, bool download) {
  Stopwatch sw;
  const int rc = gz_quantize(ctx_, &q[0][0], download ? sc_.img.data() : nullptr);
  timer_[kTQuant] += sw.lap();
  if (rc != GZ_OK) return Fail("gz_quantize", rc);
  memcpy(quant_, q, sizeof(QuantMatrix));
  return true;
}

bool Encoder::TryMatrix(float target_mul, const QuantMatrix q, Trial* t) {   // :298-326
  memcpy(t->q, q, sizeof(QuantMatrix));
  if (!SetImageFromQuantization(q, false)) return false;
  SymbolHistogram dc[3], ac[3];
  size_t size = 0;
  if (!DeviceHistograms(q, dc, ac) || !CompareBegin() || !Serialize(q, dc, ac, &size)) return false;
  Log("Iter %2d: %s quantization matrix:\n", stats_->counters[kNumItersCnt] + 1, FrameStr());
  LogMatrix(q);
  Log("Iter %2d: %s GQ[%5.2f] Out[%7zd]", stats_->counters[kNumItersCnt] + 1, FrameStr(),
      HeuristicScore(q), size);
  ++stats_->counters[kNumItersCnt];
  if (!CompareCurrent()) return false;
  t->dist_ok = DistanceOK(target_mul);
  t->jpg_size = size;
  return MaybeOutput(size);
}

bool Encoder::SelectMatrix(QuantMatrix best_q, bool downsample, bool* dist_ok) {   // SelectQuantMatrix, :328-360
  MatrixSearch search(downsample);
  const float target_mul_high = 0.97f, target_mul_low = 0.95f;
  Trial best;
  if (!TryMatrix(target_mul_high, best_q, &best)) return false;
  for (;;) {
    QuantMatrix next;
    if (!search.Next(next)) break;
    Trial t;
    if (!TryMatrix(target_mul_high, next, &t)) return false;
    search.Add(t);
    const bool better = t.dist_ok != best.dist_ok ? t.dist_ok : t.jpg_size < best.jpg_size;
    if (better) {
      best = t;
      if (t.dist_ok && !DistanceOK(target_mul_low)) break;
    }
  }
  memcpy(best_q, best.q, sizeof(QuantMatrix));
  Log("\n%s selected quantization matrix:\n", downsample ? "YUV420" : "YUV444");
  LogMatrix(best_q);
  *dist_ok = best.dist_ok;
  return true;
}

}  // namespace guetzli_amd
