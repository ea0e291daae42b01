// JPEG input: baseline / extended-sequential / progressive Huffman JPEG
// -> quantised DCT coefficients + tables + metadata, what guetzli::ReadJpeg(data,
// JPEG_READ_ALL, &jpg) (jpeg_data_reader.cc:931-1073) leaves in JPEGData for
// guetzli::Process(params, stats, jpeg_data, &out) (processor.cc:890-924).
//
// Written from ITU-T T.81: marker parsing (B.2), Huffman table construction (C),
// sequential decoding (F.2.2) and progressive decoding with successive approximation
// (G.1.2), restart intervals (E.2.4).  Host code: parsing an entropy-coded stream is serial.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <functional>
#include <string>
#include <vector>

namespace guetzli_amd {

struct JpegQuant {
  int values[64];   // natural (row-major) order
  int precision;    // 0: 8 bit, 1: 16 bit
  int index;        // Tq, 0..3
};

struct JpegComponentIn {
  int id = 0;
  int h_samp = 1, v_samp = 1;
  int quant_idx = 0;                 // position in JpegInput::quant (after FixupIndexes, :890-909)
  int width_in_blocks = 0, height_in_blocks = 0;
  std::vector<int16_t> coeffs;       // [height_in_blocks][width_in_blocks][64], quantised
};

struct JpegInput {
  int width = 0, height = 0;
  int max_h_samp = 1, max_v_samp = 1;
  int mcu_rows = 0, mcu_cols = 0;
  int restart_interval = 0;
  bool progressive = false;
  std::vector<JpegComponentIn> components;
  std::vector<JpegQuant> quant;         // every DQT table in file order (:346-375)
  std::vector<std::string> app_data;    // marker byte + segment (length included), :396-408
  std::vector<std::string> com_data;    // segment with its length bytes, :411-422
  std::string tail_data;                // bytes after EOI (:1046-1049)
  bool scan_decoded_elsewhere = false;  // a ScanDecoder took the scan: `coeffs` of the components are EMPTY (never allocated)
  bool stopped_at_scan = false;         // a ScanDecoder ended the parse at its scan (kScanDecoderStop): the headers in front of it, no more

  bool Is444() const;                   // jpeg_data.cc:36-46
  bool Is420() const;                   // jpeg_data.cc:24-34
};

// An "eligible" scan as the reader hands it to a scan decoder: a sequential 8-bit frame, ONE scan that names all of the
// frame's components in frame order, one component sampled 1 x 1 or three sampled 4:4:4 or 4:2:0, no restart interval in
// force, every quantisation table already seen.  The header checks, the progression bookkeeping and the table checks of
// the scan have passed; what is left is the block loop.
struct ScanRequest {
  int width = 0, height = 0, ncomp = 0, chroma_factor = 1;
  const uint8_t* data = nullptr;   // from the first byte behind the SOS header ...
  size_t len = 0;                  // ... to the end of the file
  struct Table { uint8_t counts[16]; uint8_t values[256]; } dc[3], ac[3];   // per component, as its DHT held them
  int quant[3][64];                // per component, natural order
  const struct JpegInput* so_far = nullptr;   // what the reader has seen in front of the scan
};
// true: the decoder has produced the scan's coefficients (dequantised, wherever its owner wants them) exactly as the
// block loop would have, and *end_offset is where BitReader::Finish would leave the parser, from `data`: the parser goes
// on there, so whatever follows gets the verdict it always got.  false: the block loop runs as if there were no decoder.
// true with *end_offset = kScanDecoderStop: the decoder only wanted to see the request (a batch collects the scans of
// many files before it decodes any).  ReadJpeg returns true at once, with JpegInput::stopped_at_scan set and nothing read
// behind the scan's header: no coefficients, no tail, none of the checks at the end of the file.
typedef std::function<bool(const ScanRequest&, size_t* end_offset)> ScanDecoder;
constexpr size_t kScanDecoderStop = (size_t)-1;

// false on anything the stream does not allow; *error (optional) gets a short description.  scan_decoder (optional) is
// offered every eligible scan.
bool ReadJpeg(const uint8_t* data, size_t len, JpegInput* jpg, std::string* error = nullptr,
              const ScanDecoder* scan_decoder = nullptr);

}  // namespace guetzli_amd
