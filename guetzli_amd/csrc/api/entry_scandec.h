// C ABI: a baseline scan read on the device (gz_decode_scan, gz_decode_scan_device) -- the four passes of
// gz_kernels_scandec.h on one stream, the host reading one word per inter-workgroup round and the verdict at the end;
// on GZ_SCAN_DECODED the coefficients go to the host, or through stage_reconstruct and k_emit_rgb into the caller's
// image without leaving the device (entry_decode.h's DecodeScratch, stream contract and argument checks).
// gz_decode_scan_input is the same call with passes 3 and 4 in their input mode: the reader's own result -- quantised
// values on grids padded to whole MCUs -- and CheckJpegSanity's verdict, for an encode of JPEG input.
// (part of the one translation unit gz_api.hip)
#pragma once

namespace {

constexpr int kScanDecDefaultSubseq = 64, kScanDecDefaultRounds = 16;

// The arguments alone: no device call.  Fills the tables and the geometry but its stream-dependent part.
int check_scan(const gz_scan* sc, ScanDecTables* T, ScanDecGeom* g, int* subseq, int* rounds) {
  if (!sc || sc->struct_size != (int)sizeof(gz_scan) || !sc->data) return GZ_E_ARG;
  if (sc->len < 3 || sc->len >= (1ull << 28)) return GZ_E_ARG;
  *subseq = sc->subseq_bytes == 0 ? kScanDecDefaultSubseq : sc->subseq_bytes;
  *rounds = sc->max_sync_rounds == 0 ? kScanDecDefaultRounds : sc->max_sync_rounds;
  if (*subseq < 16 || *subseq > 1024 || *subseq % 4 != 0) return GZ_E_ARG;
  if (*rounds < 1 || *rounds > (1 << 20)) return GZ_E_ARG;
  if (sc->ncomp != 1 && sc->ncomp != 3) return GZ_E_ARG;
  if (sc->chroma_factor != 1 && !(sc->chroma_factor == 2 && sc->ncomp == 3)) return GZ_E_ARG;
  if (sc->w <= 0 || sc->h <= 0 || sc->w >= (1 << 16) || sc->h >= (1 << 16)) return GZ_E_ARG;
  const int f = sc->chroma_factor;
  const int mcu_cols = (sc->w + 8 * f - 1) / (8 * f), mcu_rows = (sc->h + 8 * f - 1) / (8 * f);
  if ((uint64_t)mcu_cols * f * (uint64_t)mcu_rows * f > (1ull << 21)) return GZ_E_ARG;   // (the reader's "image too large")
  memset(T, 0, sizeof(*T));
  for (int c = 0; c < sc->ncomp; ++c) {
    if (!scandec_build_table(T, c, false, sc->dc[c].counts, sc->dc[c].values)) return GZ_E_ARG;
    if (!scandec_build_table(T, 3 + c, true, sc->ac[c].counts, sc->ac[c].values)) return GZ_E_ARG;
    for (int k = 0; k < 64; ++k) {
      if (sc->quant[c][k] < 1 || sc->quant[c][k] > 65535) return GZ_E_ARG;
      T->quant[c][k] = sc->quant[c][k];
    }
  }
  g->units = sc->ncomp == 1 ? 1 : f == 2 ? 6 : 3;
  g->mcu_cols = mcu_cols;
  g->total = mcu_cols * mcu_rows * g->units;
  g->bw = (sc->w + 7) / 8; g->bh = (sc->h + 7) / 8;
  g->cbw = mcu_cols; g->cbh = mcu_rows;
  g->subseq_bytes = *subseq;
  return GZ_OK;
}

// The scratch of a call as one allocation, its parts 16-byte aligned.
struct ScanDecLayout {
  size_t tables, data, entry, exit, off, bnd, count, zeroed, changed, scan_state, dcd, zeroed_end, res, total;
};
ScanDecLayout scandec_layout(size_t upload, int nsub, int nwg, int rounds, int total_blocks, size_t state_bytes) {
  ScanDecLayout l;
  size_t at = 0;
  auto take = [&at](size_t bytes) { const size_t p = at; at += (bytes + 15) & ~(size_t)15; return p; };
  l.tables = take(sizeof(ScanDecTables));
  l.data = take(upload);
  l.entry = take(8 * (size_t)nsub);
  l.exit = take(8 * (size_t)nsub);
  l.off = take(8 * ((size_t)nsub + 1));
  l.bnd = take(8 * 2 * (size_t)nwg);
  l.count = take(4 * (size_t)nsub);
  l.zeroed = at;                       // one fill: the rounds' words, k_scan_offsets' scratch, the DC differences
  l.changed = take(4 * ((size_t)rounds + 1));
  l.scan_state = take(state_bytes);
  l.dcd = take(2 * (size_t)total_blocks);
  l.zeroed_end = at;
  l.res = take(16);
  l.total = at;
  return l;
}

// host_input (with large_coeff): the input mode, g.total * 64 values; otherwise `out` and / or host_coeffs.
int decode_scan(int device, const gz_scan* sc, const ScanDecTables& T, ScanDecGeom g, int rounds, const gz_device_output* out,
                int16_t* host_coeffs, int16_t* host_input, int* large_coeff, gz_scan_result* result) {
  const int w = sc->w, h = sc->h;
  if (probe_device(device) != GZ_OK) return GZ_E_NO_DEVICE;
  if (out && check_tensor_memory(device, tensor_view(out, w, h), "data", nullptr) != GZ_OK) return GZ_E_ARG;
  const size_t end = scandec_data_end(sc->data, (size_t)sc->len);
  g.end_bits = (unsigned)(end * 8);
  g.nsub = std::max(1, (int)((end + (size_t)g.subseq_bytes - 1) / (size_t)g.subseq_bytes));
  const int nwg = gz_div_up(g.nsub, kScanDecLanes);
  result->subsequences = g.nsub;
  DecodeScratch s;
  gz_ctx* c = &s.t;
  s.set_frame_geometry(device, w, h, sc->chroma_factor);
  const int max_tiles = gz_div_up(g.nsub, kScanTile) + 1;
  const size_t upload = std::max<size_t>(end, 1);
  const ScanDecLayout l = scandec_layout(upload, g.nsub, nwg, rounds, g.total, scan_state_bytes(max_tiles));
  // the decoder's scratch and the coefficients, and for pixels what gz_decode_coeffs_device takes: all of them or none
  const size_t coeff_bytes = host_input ? (size_t)g.total * 128 : (size_t)c->nblk * 128;
  if (host_input) {
    TRY(regrow(c, nullptr, nullptr, 0, {{(void**)&s.d_scan, l.total}, {(void**)&c->d_cand, coeff_bytes}}));
  } else if (!out) {
    TRY(regrow(c, nullptr, nullptr, 0, {{(void**)&s.d_scan, l.total}, {(void**)&c->d_cand, (size_t)c->nblk * 128}}));
  } else if (sc->chroma_factor == 2) {
    TRY(regrow(c, nullptr, nullptr, 0, {{(void**)&s.d_scan, l.total}, {(void**)&c->d_cand, (size_t)c->nblk * 128},
                                        {(void**)&c->d_srgb_out, (size_t)3 * w * h}, {(void**)&s.d_lut, sizeof(float) * 256},
                                        {(void**)&c->d_csamp, 2 * csamp_plane(c)}}));
  } else {
    TRY(regrow(c, nullptr, nullptr, 0, {{(void**)&s.d_scan, l.total}, {(void**)&c->d_cand, (size_t)c->nblk * 128},
                                        {(void**)&c->d_srgb_out, (size_t)3 * w * h}, {(void**)&s.d_lut, sizeof(float) * 256}}));
  }
  uint8_t* const d = s.d_scan;
  hipStream_t stream = nullptr;
  TRY(s.open_streams(&stream));
  const ScanDecTables* d_T = (const ScanDecTables*)(d + l.tables);
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
  HIPCHK(c, hipMemcpyAsync(d + l.tables, &T, sizeof(T), hipMemcpyHostToDevice, stream));
  if (end > 0) HIPCHK(c, hipMemcpyAsync(d + l.data, sc->data, end, hipMemcpyHostToDevice, stream));
  HIPCHK(c, hipMemsetAsync(d + l.zeroed, 0, l.zeroed_end - l.zeroed, stream));
  HIPCHK(c, hipMemsetAsync(d_res, 0xff, 16, stream));
  if (host_input) HIPCHK(c, hipMemsetAsync(d_res + 2, 0, 8, stream));   // (the large-coefficient word)
  HIPCHK(c, hipMemsetAsync(c->d_cand, 0, coeff_bytes, stream));
  // 1. synchronise
  launch_scandec_sync_first(stream, d_data, d_T, g, st, d_bnd);
  KCHK(c);
  int used = 0;
  bool converged = nwg == 1;
  while (!converged && used < rounds) {
    ++used;
    launch_scandec_sync_next(stream, d_data, d_T, g, st, d_bnd + (size_t)((used - 1) & 1) * nwg, d_bnd + (size_t)(used & 1) * nwg, d_changed + used);
    KCHK(c);
    unsigned changed = 1;
    HIPCHK(c, hipMemcpyAsync(&changed, d_changed + used, sizeof(changed), hipMemcpyDeviceToHost, stream));
    HIPCHK(c, hipStreamSynchronize(stream));
    converged = changed == 0;
  }
  result->sync_rounds = used;
  if (!converged) {
    s.idle = true;
    result->status = GZ_SCAN_NOT_CONVERGED;
    return GZ_OK;
  }
  // 2. offsets (the scratch is zero: epoch 1)
  GZ_LAUNCH(k_scan_offsets, dim3(std::max(1, gz_div_up(g.nsub, kScanTile))), dim3(256), stream, (const unsigned*)st.count, g.nsub, d_off,
            scan_state_at(d + l.scan_state, max_tiles), 1u);
  KCHK(c);
  // 3. write, 4. DC
  if (host_input) launch_scandec_write_input(stream, d_data, d_T, g, st.entry, d_off, c->d_cand, d_dcd, d_res);
  else launch_scandec_write(stream, d_data, d_T, g, st.entry, d_off, c->d_cand, d_dcd, d_res);
  KCHK(c);
  if (host_input) launch_scandec_dc_input(stream, sc->ncomp, d_dcd, d_T, g, c->d_cand, d_res);
  else launch_scandec_dc(stream, sc->ncomp, d_dcd, d_T, g, c->d_cand, d_res);
  KCHK(c);
  unsigned res[3] = {0, 0, 0};
  HIPCHK(c, hipMemcpyAsync(res, d_res, host_input ? 12 : 8, hipMemcpyDeviceToHost, stream));
  HIPCHK(c, hipStreamSynchronize(stream));
  s.idle = true;
  if (res[0] != 0xffffffffu) {
    static const int kStatus[8] = {GZ_SCAN_BAD_SYMBOL, GZ_SCAN_BAD_SYMBOL, GZ_SCAN_RUN_PAST_BAND, GZ_SCAN_DC_RANGE, GZ_SCAN_COEFF_RANGE,
                                   GZ_SCAN_ENDS_EARLY, GZ_SCAN_BAD_SYMBOL, GZ_SCAN_BAD_SYMBOL};
    result->status = kStatus[res[0] & 7u];
    return GZ_OK;
  }
  if (res[1] == 0xffffffffu || res[1] > g.end_bits) {   // the data end before the last block does
    result->status = GZ_SCAN_ENDS_EARLY;
    return GZ_OK;
  }
  // BitReader::Finish: whole unread bytes go back, a stuffed pair as one
  size_t pos = ((size_t)res[1] + 7) / 8;
  if ((res[1] & 7u) != 0 && pos < end && sc->data[pos - 1] == 0xff) ++pos;
  result->end_offset = pos;
  s.idle = false;
  if (host_coeffs) HIPCHK(c, hipMemcpyAsync(host_coeffs, c->d_cand, (size_t)c->nblk * 128, hipMemcpyDeviceToHost, stream));
  if (host_input) HIPCHK(c, hipMemcpyAsync(host_input, c->d_cand, coeff_bytes, hipMemcpyDeviceToHost, stream));
  if (out) {
    TRY(outputs_after_consumers(c, stream, &s.ev, {out->consumer_stream}));
    TRY(stage_reconstruct(c, stream, c->d_cand, nullptr, c->d_srgb_out));
    if (tensor_float_dtype(out->dtype))
      HIPCHK(c, hipMemcpyAsync(s.d_lut, emit_lut(), sizeof(float) * 256, hipMemcpyHostToDevice, stream));
    launch_emit(stream, c->d_srgb_out, w, h, out, s.d_lut);
    KCHK(c);
    TRY(consumers_after_outputs(c, stream, s.ev, {out->consumer_stream}));
  }
  HIPCHK(c, hipStreamSynchronize(stream));   // (the temporaries go back to the pool behind this)
  s.idle = true;
  if (host_input) *large_coeff = res[2] != 0 ? 1 : 0;
  result->status = GZ_SCAN_DECODED;
  return GZ_OK;
}

int decode_scan_entry(int device, const gz_scan* sc, const gz_device_output* out, int16_t* host_coeffs, int16_t* host_input,
                      int* large_coeff, gz_scan_result* result) {
  if (!result) return GZ_E_ARG;
  memset(result, 0, sizeof(*result));
  result->status = GZ_SCAN_NOT_CONVERGED;   // (until a verdict is reached)
  // (static thread_local: 10 KB of tables the kernels' argument checks fill)
  static thread_local ScanDecTables T;
  ScanDecGeom g;
  memset(&g, 0, sizeof(g));
  int subseq = 0, rounds = 0;
  if (const int rc = check_scan(sc, &T, &g, &subseq, &rounds)) return rc;
  if (out && check_device_output(out, sc->w, sc->h) != GZ_OK) return GZ_E_ARG;
  CallerDevice keep(device);
  return decode_scan(device, sc, T, g, rounds, out, host_coeffs, host_input, large_coeff, result);
}
}  // namespace

extern "C" {

int gz_decode_scan(int device, const gz_scan* scan, int16_t* host_coeffs, gz_scan_result* result) {
  if (!host_coeffs) return GZ_E_ARG;
  return decode_scan_entry(device, scan, nullptr, host_coeffs, nullptr, nullptr, result);
}

int gz_decode_scan_device(int device, const gz_scan* scan, const gz_device_output* out, gz_scan_result* result) {
  if (!out) return GZ_E_ARG;
  return decode_scan_entry(device, scan, out, nullptr, nullptr, nullptr, result);
}

int gz_decode_scan_input(int device, const gz_scan* scan, int16_t* host_coeffs, int* large_coeff, gz_scan_result* result) {
  if (!host_coeffs || !large_coeff) return GZ_E_ARG;
  return decode_scan_entry(device, scan, nullptr, nullptr, host_coeffs, large_coeff, result);
}

}  // extern "C"
