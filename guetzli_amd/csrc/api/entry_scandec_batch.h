// C ABI: gz_decode_scan_batch_device -- n baseline scans of one frame size through the launches of ONE device decode.
// The passes are entry_scandec.h's, each launched once for a chunk of scans (gz_kernels_scandec.h: the batched forms,
// the layout of a batch); the host reads one word per scan and synchronisation round, and the verdicts at the end; the
// scans that decoded leave through the batched forms of the reconstruction kernels and of k_emit_rgb, which take the
// list of them.  Results and pixels of scan i are gz_decode_scan_device's for that scan alone.
// (part of the one translation unit gz_api.hip, which includes these files in order -- no declaration here is visible
// outside libguetzli_amd.so but the C ABI)
#pragma once

namespace {

constexpr int kScanBatchMaxImages = 65535;   // gridDim.y of the DC pass and of the pixel kernels

// What the call knows of scan i before any device call.
struct ScanBatchItem {
  ScanDecGeom g;       // complete: end_bits and nsub included
  size_t end;          // bytes of the stream the decoder may read
  int nwg;
};
// Sums over the scans of a chunk: what its scratch is sized by.
struct ScanBatchSums {
  size_t m = 0, upload = 0, lanes = 0, wgs = 0, blocks = 0;
  void add(const ScanBatchItem& it) {
    ++m;
    upload += (std::max<size_t>(it.end, 1) + 15) & ~(size_t)15;
    lanes += (size_t)it.nwg * kScanDecLanes;
    wgs += (size_t)it.nwg;
    blocks += (size_t)it.g.total;
  }
};
// The decoder's scratch of a chunk as one allocation, its parts 16-byte aligned.  [tables, upload_end) is one upload.
struct ScanBatchLayout {
  size_t tables, images, wg_image, data, upload_end, entry, exit, off, bnd, zeroed, count, changed, scan_state, dcd, zeroed_end, res, list, total;
};
ScanBatchLayout scan_batch_layout(const ScanBatchSums& s) {
  ScanBatchLayout l;
  size_t at = 0;
  auto take = [&at](size_t bytes) { const size_t p = at; at += (bytes + 15) & ~(size_t)15; return p; };
  l.tables = take(sizeof(ScanDecTables) * s.m);
  l.images = take(sizeof(ScanDecImage) * s.m);
  l.wg_image = take(4 * s.wgs);
  l.data = take(s.upload);
  l.upload_end = at;
  l.entry = take(8 * s.lanes);
  l.exit = take(8 * s.lanes);
  l.off = take(8 * (s.lanes + 1));
  l.bnd = take(8 * 2 * s.wgs);
  l.zeroed = at;                       // one fill: the padded lanes' counts, the round's words, k_scan_offsets' scratch, the DC differences
  l.count = take(4 * s.lanes);
  l.changed = take(4 * s.m);
  l.scan_state = take(scan_state_bytes(gz_div_up((int)s.lanes, kScanTile) + 1));
  l.dcd = take(2 * s.blocks);
  l.zeroed_end = at;
  l.res = take(16 * s.m);
  l.list = take(4 * 2 * s.m);          // the decoded scans: their arenas, their slots
  l.total = at;
  return l;
}
// The frame's scratch of one image: its coefficient arena, its packed pixels, its chroma samples (4:2:0).
struct ScanBatchFrame {
  size_t coeff_bytes, srgb_stride, samp_stride;
  size_t per_image() const { return coeff_bytes + srgb_stride + samp_stride; }
};
size_t scan_batch_bytes(const ScanBatchSums& s, const ScanBatchFrame& f) {
  return scan_batch_layout(s).total + s.m * f.per_image() + sizeof(float) * 256;
}

// The verdict of one scan from its two result words, as decode_scan reads them.
void scan_batch_verdict(const gz_scan* sc, const ScanBatchItem& it, const unsigned* res, gz_scan_result* result) {
  if (res[0] != 0xffffffffu) {
    static const int kStatus[8] = {GZ_SCAN_BAD_SYMBOL, GZ_SCAN_BAD_SYMBOL, GZ_SCAN_RUN_PAST_BAND, GZ_SCAN_DC_RANGE, GZ_SCAN_COEFF_RANGE,
                                   GZ_SCAN_ENDS_EARLY, GZ_SCAN_BAD_SYMBOL, GZ_SCAN_BAD_SYMBOL};
    result->status = kStatus[res[0] & 7u];
    return;
  }
  if (res[1] == 0xffffffffu || res[1] > it.g.end_bits) {   // the data end before the last block does
    result->status = GZ_SCAN_ENDS_EARLY;
    return;
  }
  // BitReader::Finish: whole unread bytes go back, a stuffed pair as one
  size_t pos = ((size_t)res[1] + 7) / 8;
  if ((res[1] & 7u) != 0 && pos < it.end && sc->data[pos - 1] == 0xff) ++pos;
  result->end_offset = pos;
  result->status = GZ_SCAN_DECODED;
}

// The batched pixel kernels on `stream`: the K listed arenas' coefficients -> their packed images -> the listed slots of out.
int scan_batch_pixels(gz_ctx* c, hipStream_t stream, int K, const int* d_arena, const int* d_slot, const ScanBatchFrame& f,
                      const gz_device_output_batch* out, const float* d_lut) {
  const int w = c->w, h = c->h;
  const size_t coeff_stride = f.coeff_bytes / 2;
  if (c->cfac == 2) {
    GZ_LAUNCH(k_chroma_samples_batch, dim3(gz_div_up(c->nbc, kBlocksPerWG), K), dim3(256), stream, (const int16_t*)c->d_cand,
              (size_t)c->coff[1] * 64, (size_t)c->coff[2] * 64, c->cbw, c->nbc, c->d_csamp, d_arena, coeff_stride, f.samp_stride);
    KCHK(c);
    GZ_LAUNCH(k_reconstruct420_batch, dim3(c->bh * gz_div_up(c->bw, 8), K), dim3(256), stream, (const int16_t*)c->d_cand,
              (const uint8_t*)c->d_csamp, w, h, c->bw, c->nb, c->cbw, c->cbh, c->d_srgb_out, d_arena, coeff_stride, f.samp_stride, f.srgb_stride);
    KCHK(c);
  } else {
    // strips per workgroup as stage_reconstruct chooses them, the launch's workgroups being those of K frames
    const int strips = gz_div_up(c->bw, kReconBlocks);
    int per = 4;
    while (per > 1 && (long)c->bh * gz_div_up(strips, per) * K < 2000) per >>= 1;
    GZ_LAUNCH(k_reconstruct_batch, dim3(c->bh * gz_div_up(strips, per), K), dim3(256), stream, (const int16_t*)c->d_cand, w, h, c->bw, c->nb,
              c->d_srgb_out, per, d_arena, coeff_stride, f.srgb_stride);
    KCHK(c);
  }
  const long long sn = out->stride_n, sy = out->stride_y, sx = out->stride_x, sc = out->stride_c;
  with_sample_type(out->dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    launch_emit_rgb_batch(stream, c->d_srgb_out, w, h, (T*)out->data, sn, sy, sx, sc, d_lut, d_arena, d_slot, K, f.srgb_stride);
  });
  KCHK(c);
  return GZ_OK;
}

// (every argument is checked; items and tables are the scans'; chunks: [first, first + count) each)
int decode_scan_batch(int device, const gz_scan* scans, const int* slots, const gz_device_output_batch* out, int rounds,
                      const std::vector<ScanBatchItem>& items, const std::vector<ScanDecTables>& tables,
                      const std::vector<std::pair<int, int>>& chunks, const ScanBatchFrame& f, gz_scan_result* results) {
  const int w = scans[0].w, h = scans[0].h, ncomp = scans[0].ncomp;
  if (probe_device(device) != GZ_OK) return GZ_E_NO_DEVICE;
  if (check_tensor_memory(device, tensor_view(out, w, h), "data", nullptr) != GZ_OK) return GZ_E_ARG;
  // the largest chunk sizes every buffer: the decoder's scratch, the arenas, the packed pixels, the chroma samples, the
  // table -- all of them or none
  size_t scan_bytes = 0, most = 0;
  for (const std::pair<int, int>& ch : chunks) {
    ScanBatchSums sums;
    for (int j = 0; j < ch.second; ++j) sums.add(items[(size_t)ch.first + j]);
    scan_bytes = std::max(scan_bytes, scan_batch_layout(sums).total);
    most = std::max(most, (size_t)ch.second);
  }
  // (host memory the copies read and write: declared in front of the scratch, whose destructor waits for the stream)
  std::vector<uint8_t> blob;
  std::vector<unsigned> words;
  std::vector<int> list;
  std::vector<gz_scan_result> verdicts;
  DecodeScratch s;
  gz_ctx* c = &s.t;
  s.set_frame_geometry(device, w, h, scans[0].chroma_factor);
  if (scans[0].chroma_factor == 2) {
    TRY(regrow(c, nullptr, nullptr, 0, {{(void**)&s.d_scan, scan_bytes}, {(void**)&c->d_cand, most * f.coeff_bytes},
                                        {(void**)&c->d_srgb_out, most * f.srgb_stride}, {(void**)&s.d_lut, sizeof(float) * 256},
                                        {(void**)&c->d_csamp, most * f.samp_stride}}));
  } else {
    TRY(regrow(c, nullptr, nullptr, 0, {{(void**)&s.d_scan, scan_bytes}, {(void**)&c->d_cand, most * f.coeff_bytes},
                                        {(void**)&c->d_srgb_out, most * f.srgb_stride}, {(void**)&s.d_lut, sizeof(float) * 256}}));
  }
  uint8_t* const d = s.d_scan;
  hipStream_t stream = nullptr;
  TRY(s.open_streams(&stream));
  bool emitted = false;
  for (const std::pair<int, int>& ch : chunks) {
    const int first = ch.first, m = ch.second;
    ScanBatchSums sums;
    for (int j = 0; j < m; ++j) sums.add(items[(size_t)first + j]);
    const ScanBatchLayout l = scan_batch_layout(sums);
    const int nwg = (int)sums.wgs, lanes = (int)sums.lanes;
    // the upload: tables, descriptors, the workgroups' images, the streams
    blob.assign(l.upload_end, 0);
    ScanDecImage* images = (ScanDecImage*)(blob.data() + l.images);
    int* wg_image = (int*)(blob.data() + l.wg_image);
    ScanBatchSums at;
    bool rounds_needed = false;
    for (int j = 0; j < m; ++j) {
      const ScanBatchItem& it = items[(size_t)first + j];
      memcpy(blob.data() + l.tables + sizeof(ScanDecTables) * (size_t)j, &tables[(size_t)first + j], sizeof(ScanDecTables));
      ScanDecImage im;
      memset(&im, 0, sizeof(im));
      im.g = it.g;
      im.data_at = at.upload;
      im.coeff_at = (unsigned long long)j * (f.coeff_bytes / 2);
      im.wg0 = (int)at.wgs;
      im.lane0 = (int)at.lanes;
      im.block0 = (int)at.blocks;
      im.nwg = it.nwg;
      images[j] = im;
      for (int k = 0; k < it.nwg; ++k) wg_image[at.wgs + (size_t)k] = j;
      if (it.end > 0) memcpy(blob.data() + l.data + at.upload, scans[first + j].data, it.end);
      rounds_needed = rounds_needed || it.nwg > 1;
      at.add(it);
    }
    s.idle = false;
    HIPCHK(c, hipMemcpyAsync(d + l.tables, blob.data(), l.upload_end, hipMemcpyHostToDevice, stream));
    HIPCHK(c, hipMemsetAsync(d + l.zeroed, 0, l.zeroed_end - l.zeroed, stream));
    HIPCHK(c, hipMemsetAsync(d + l.res, 0xff, 16 * (size_t)m, stream));
    HIPCHK(c, hipMemsetAsync(c->d_cand, 0, (size_t)m * f.coeff_bytes, stream));
    const ScanDecTables* d_T = (const ScanDecTables*)(d + l.tables);
    const ScanDecImage* d_images = (const ScanDecImage*)(d + l.images);
    const int* d_wg_image = (const int*)(d + l.wg_image);
    const uint8_t* d_data = d + l.data;
    ScanDecState st;
    st.entry = (unsigned long long*)(d + l.entry);
    st.exit = (unsigned long long*)(d + l.exit);
    st.count = (unsigned*)(d + l.count);
    unsigned long long* d_off = (unsigned long long*)(d + l.off);
    unsigned long long* d_bnd = (unsigned long long*)(d + l.bnd);
    unsigned* d_changed = (unsigned*)(d + l.changed);
    unsigned* d_res = (unsigned*)(d + l.res);
    int16_t* d_dcd = (int16_t*)(d + l.dcd);
    verdicts.assign((size_t)m, gz_scan_result());
    for (int j = 0; j < m; ++j) {
      memset(&verdicts[(size_t)j], 0, sizeof(gz_scan_result));
      verdicts[(size_t)j].status = GZ_SCAN_NOT_CONVERGED;
      verdicts[(size_t)j].subsequences = items[(size_t)first + j].g.nsub;
    }
    // 1. synchronise: a round for all while any scan's word is set; a scan's rounds are those up to its first zero word
    launch_scandec_sync_first_batch(stream, nwg, d_data, d_T, d_images, d_wg_image, st, d_bnd);
    KCHK(c);
    std::vector<char> converged((size_t)m);
    int open = 0, used = 0;
    for (int j = 0; j < m; ++j) {
      converged[(size_t)j] = items[(size_t)first + j].nwg == 1;
      open += converged[(size_t)j] ? 0 : 1;
    }
    words.assign((size_t)m, 1u);
    while (open > 0 && used < rounds) {
      ++used;
      if (used > 1) HIPCHK(c, hipMemsetAsync(d_changed, 0, 4 * (size_t)m, stream));
      launch_scandec_sync_next_batch(stream, nwg, d_data, d_T, d_images, d_wg_image, st, d_bnd + (size_t)((used - 1) & 1) * nwg,
                                     d_bnd + (size_t)(used & 1) * nwg, d_changed);
      KCHK(c);
      HIPCHK(c, hipMemcpyAsync(words.data(), d_changed, 4 * (size_t)m, hipMemcpyDeviceToHost, stream));
      HIPCHK(c, hipStreamSynchronize(stream));
      for (int j = 0; j < m; ++j) {
        if (converged[(size_t)j]) continue;
        verdicts[(size_t)j].sync_rounds = used;
        if (words[(size_t)j] == 0) { converged[(size_t)j] = 1; --open; }
      }
    }
    if (open < m) {
      // 2. offsets over all padded lanes (the scratch is zero: epoch 1)
      const int max_tiles = gz_div_up(lanes, kScanTile) + 1;
      GZ_LAUNCH(k_scan_offsets, dim3(std::max(1, gz_div_up(lanes, kScanTile))), dim3(256), stream, (const unsigned*)st.count, lanes, d_off,
                scan_state_at(d + l.scan_state, max_tiles), 1u);
      KCHK(c);
      // 3. write, 4. DC: of every scan (one that did not converge is decoded from the states it has, into its own arena,
      // and its result words are not read)
      launch_scandec_write_batch(stream, nwg, d_data, d_T, d_images, d_wg_image, st.entry, d_off, c->d_cand, d_dcd, d_res);
      KCHK(c);
      launch_scandec_dc_batch(stream, ncomp, m, d_dcd, d_T, d_images, c->d_cand, d_res);
      KCHK(c);
      words.assign(4 * (size_t)m, 0u);
      HIPCHK(c, hipMemcpyAsync(words.data(), d_res, 16 * (size_t)m, hipMemcpyDeviceToHost, stream));
      HIPCHK(c, hipStreamSynchronize(stream));
      list.assign(2 * (size_t)m, 0);
      int K = 0;
      for (int j = 0; j < m; ++j) {
        if (!converged[(size_t)j]) continue;
        scan_batch_verdict(&scans[first + j], items[(size_t)first + j], &words[4 * (size_t)j], &verdicts[(size_t)j]);
        if (verdicts[(size_t)j].status != GZ_SCAN_DECODED) continue;
        list[(size_t)K] = j;
        list[(size_t)m + (size_t)K] = slots[first + j];
        ++K;
      }
      if (K > 0) {
        int* d_list = (int*)(d + l.list);
        HIPCHK(c, hipMemcpyAsync(d_list, list.data(), 4 * 2 * (size_t)m, hipMemcpyHostToDevice, stream));
        if (!emitted) {
          TRY(outputs_after_consumers(c, stream, &s.ev, {out->consumer_stream}));
          if (tensor_float_dtype(out->dtype))
            HIPCHK(c, hipMemcpyAsync(s.d_lut, emit_lut(), sizeof(float) * 256, hipMemcpyHostToDevice, stream));
          emitted = true;
        }
        TRY(scan_batch_pixels(c, stream, K, d_list, d_list + m, f, out, s.d_lut));
        // (the consumer's stream goes on behind this chunk's pixels: a later chunk that fails leaves these ordered)
        TRY(consumers_after_outputs(c, stream, s.ev, {out->consumer_stream}));
        HIPCHK(c, hipStreamSynchronize(stream));   // (the next chunk's uploads overwrite the list and the streams)
      }
    }
    s.idle = true;
    for (int j = 0; j < m; ++j) results[first + j] = verdicts[(size_t)j];
  }
  return GZ_OK;
}

}  // namespace

extern "C" {

int gz_decode_scan_batch_device(int device, int n, const gz_scan* scans, const int* slots, const gz_device_output_batch* out,
                                gz_scan_result* results, size_t scratch_cap_bytes) {
  // all of these before any device call
  if (n < 1 || !scans || !slots || !out || !results) return GZ_E_ARG;
  for (int i = 0; i < n; ++i) {
    memset(&results[i], 0, sizeof(results[i]));
    results[i].status = GZ_SCAN_NOT_CONVERGED;   // (until a verdict is reached)
  }
  std::vector<ScanDecTables> tables((size_t)n);
  std::vector<ScanBatchItem> items((size_t)n);
  int subseq = 0, rounds = 0;
  for (int i = 0; i < n; ++i) {
    int sb = 0, rd = 0;
    memset(&items[(size_t)i].g, 0, sizeof(ScanDecGeom));
    if (const int rc = check_scan(&scans[i], &tables[(size_t)i], &items[(size_t)i].g, &sb, &rd)) return rc;
    if (i == 0) { subseq = sb; rounds = rd; }
    if (sb != subseq || rd != rounds) return GZ_E_ARG;
    if (scans[i].w != scans[0].w || scans[i].h != scans[0].h || scans[i].ncomp != scans[0].ncomp ||
        scans[i].chroma_factor != scans[0].chroma_factor) return GZ_E_ARG;
  }
  const int w = scans[0].w, h = scans[0].h, factor = scans[0].chroma_factor;
  if (check_device_output_batch(out, w, h) != GZ_OK) return GZ_E_ARG;
  {
    std::vector<int> sorted(slots, slots + n);
    std::sort(sorted.begin(), sorted.end());
    if (sorted.front() < 0 || sorted.back() >= out->n) return GZ_E_ARG;
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return GZ_E_ARG;
  }
  // the streams' ends, lanes and workgroups; the frame's scratch per image
  for (int i = 0; i < n; ++i) {
    ScanBatchItem& it = items[(size_t)i];
    it.end = scandec_data_end(scans[i].data, (size_t)scans[i].len);
    it.g.end_bits = (unsigned)(it.end * 8);
    it.g.nsub = std::max(1, (int)((it.end + (size_t)it.g.subseq_bytes - 1) / (size_t)it.g.subseq_bytes));
    it.nwg = gz_div_up(it.g.nsub, kScanDecLanes);
  }
  ScanBatchFrame f;
  {
    const size_t nb = (size_t)((w + 7) / 8) * ((h + 7) / 8);
    const size_t nbc = (size_t)((w + 8 * factor - 1) / (8 * factor)) * ((h + 8 * factor - 1) / (8 * factor));
    f.coeff_bytes = (nb + 2 * nbc) * 128;
    f.srgb_stride = ((size_t)3 * w * h + 15) & ~(size_t)15;
    f.samp_stride = factor == 2 ? 2 * (size_t)((w + 15) / 16 * 8) * (size_t)((h + 15) / 16 * 8) : 0;   // (2 csamp_plane)
  }
  // chunks: consecutive scans, as many as the cap holds and the grid can index; a scan that does not fit alone is refused
  const size_t cap = scratch_cap_bytes ? scratch_cap_bytes : kBatchDefaultScratch;
  std::vector<std::pair<int, int>> chunks;
  for (int first = 0; first < n;) {
    ScanBatchSums sums;
    int m = 0;
    while (first + m < n && m < kScanBatchMaxImages) {
      ScanBatchSums with = sums;
      with.add(items[(size_t)first + m]);
      if (with.lanes > (size_t)0x7fffff00 || with.blocks > (size_t)0x7fffff00) break;   // (lane and block indices are ints)
      if (scan_batch_bytes(with, f) > cap) break;
      sums = with;
      ++m;
    }
    if (m == 0) return GZ_E_ARG;
    chunks.push_back({first, m});
    first += m;
  }
  CallerDevice keep(device);
  return decode_scan_batch(device, scans, slots, out, rounds, items, tables, chunks, f, results);
}

}  // extern "C"
