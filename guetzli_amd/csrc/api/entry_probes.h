// C ABI: gz_probe_* -- stage probes for the tests (localise a divergence to one stage of the chain; the device's IEEE arithmetic and std::sort restatements).  Diagnostics, not part of any encode: -DGZ_NO_PROBES leaves them out of a deployment build.
// (part of the one translation unit gz_api.hip, which includes these files in order; split by
// concern in round 5 -- no declaration here is visible outside libguetzli_amd.so but the C ABI)
#pragma once

extern "C" {

#ifndef GZ_NO_PROBES

// ------------------------------------------------------------------- stage probes -----
int gz_probe_blur(gz_ctx* c, const float* in, float sigma, float border_ratio, float* out) {
  DeviceScope ds_(c);
  if (!c || !in || !out) return GZ_E_ARG;
  BlurCfg cfg;   // a local: its scales are this call's, freed below on every path, and never enter the context's record
  int rc = setup_blur_cfg(c, &cfg, sigma, border_ratio, false);
  float* src = c->xyb[0];
  c->xyb_is_cand = false;   // (xyb[] as scratch)
  if (rc == GZ_OK) rc = upload_planes(c, in, &src, 1);
  SrcPack<SrcPlain, 1> s; s.s[0].p = src;
  PostStore<1> post; post.out[0] = c->xyb[1];
  // the same kernels gz_compare uses for each radius: fused below 16, two passes from 16 up
  if (rc == GZ_OK) rc = blur_plane(c, c->stream, s, c->tmp[0], post, cfg);
  if (rc == GZ_OK) rc = download_plane(c, c->xyb[1], out);
  (void)hipStreamSynchronize(c->stream);
  (void)pool_free(cfg.d_scale);
  return rc;
}

int gz_probe_opsin(gz_ctx* c, const float* rgb3, float* xyb3) {
  DeviceScope ds_(c);
  if (!c || !rgb3 || !xyb3) return GZ_E_ARG;
  c->lin_is_cand = c->xyb_is_cand = false;
  TRY(upload_planes(c, rgb3, c->lin, 3));
  TRY(stage_opsin(c, c->stream));
  for (int i = 0; i < 3; ++i) TRY(download_plane(c, c->xyb[i], xyb3 + (size_t)i * c->w * c->h));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GZ_OK;
}

int gz_probe_separate_frequencies(gz_ctx* c, const float* xyb3, float* out10) {
  DeviceScope ds_(c);
  if (!c || !xyb3 || !out10) return GZ_E_ARG;
  TRY(ensure_pip(c));
  c->xyb_is_cand = false;
  TRY(upload_planes(c, xyb3, c->xyb, 3));
  TRY(stage_separate(c, chain_streams(c, false), &c->pip));
  const size_t n = (size_t)c->w * c->h;
  for (int i = 0; i < 3; ++i) TRY(download_plane(c, c->pip.lfv[i], out10 + i * n));
  for (int i = 0; i < 2; ++i) TRY(download_plane(c, c->pip.mf[i], out10 + (3 + i) * n));
  memset(out10 + 5 * n, 0, sizeof(float) * n);   // mf[2]: dead in the reference, not computed
  for (int i = 0; i < 2; ++i) TRY(download_plane(c, c->pip.hf[i], out10 + (6 + i) * n));
  for (int i = 0; i < 2; ++i) TRY(download_plane(c, c->pip.uhf[i], out10 + (8 + i) * n));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GZ_OK;
}

int gz_probe_diffmap(gz_ctx* c, const float* rgb0, const float* rgb1, float* diffmap,
                     float* score) {
  DeviceScope ds_(c);
  if (!c || !rgb0 || !rgb1) return GZ_E_ARG;
  TRY(ensure_pip(c));
  c->lin_is_cand = c->xyb_is_cand = false;
  TRY(upload_planes(c, rgb0, c->lin, 3));
  TRY(stage_opsin(c, c->stream));
  TRY(stage_separate(c, chain_streams(c, false), &c->pip));
  TRY(upload_planes(c, rgb1, c->lin, 3));
  TRY(stage_opsin(c, c->stream));
  TRY(stage_separate(c, chain_streams(c, false), &c->pi1));
  // (the diffmap stage alone takes the side streams, by the context's stream mode; no block maxima)
  TRY(stage_diffmap(c, chain_streams(c, !single_stream_wanted(c)), c->pip, c->pi1, kWantDistmap, ClearMax::kMemset));
  if (diffmap) TRY(download_plane(c, c->distmap, diffmap));
  unsigned bits = 0;
  HIPCHK(c, hipMemcpyAsync(&bits, c->d_max_bits, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (score) memcpy(score, &bits, 4);
  return GZ_OK;
}

int gz_probe_mask(gz_ctx* c, const float* xyb0, const float* xyb1, float* mask3,
                  float* mask_dc3) {
  DeviceScope ds_(c);
  if (!c || !xyb0 || !xyb1 || !mask3) return GZ_E_ARG;
  TRY(ensure_pip(c));
  // Mask(xyb0, xyb1) reads planes 0 and 1 of each image unchanged (butteraugli.cc:1765,1777)
  float* a[2] = {c->pip.hf[0], c->pip.hf[1]};
  float* b[2] = {c->pi1.hf[0], c->pi1.hf[1]};
  TRY(upload_planes(c, xyb0, a, 2));
  TRY(upload_planes(c, xyb1, b, 2));
  const float* const ca2[2] = {a[0], a[1]};
  const float* const cb2[2] = {b[0], b[1]};
  MaskPrePack pk;
  TRY(mask_pack_plain(c, c->stream, ca2, cb2, &pk));
  TRY(stage_mask_blurs(c, c->stream, c->stream, pk));
  TRY(launch_combine(c, c->stream, combine_mask_args(c, c->mask_out, c->mask_dc_out)));
  const size_t n = (size_t)c->w * c->h;
  for (int i = 0; i < 3; ++i) {
    TRY(download_plane(c, c->mask_out[i], mask3 + i * n));
    if (mask_dc3) TRY(download_plane(c, c->mask_dc_out[i], mask_dc3 + i * n));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GZ_OK;
}


int gz_probe_idct_blocks(int device, const int16_t* blocks, int n, uint8_t* out) {
  if (!blocks || !out || n <= 0) return GZ_E_ARG;
  if (probe_device(device) != GZ_OK) return GZ_E_NO_DEVICE;
  int16_t* d_in = nullptr; uint8_t* d_out = nullptr;
  if (hipMalloc((void**)&d_in, (size_t)n * 128) != hipSuccess) return GZ_E_HIP;
  if (hipMalloc((void**)&d_out, (size_t)n * 64) != hipSuccess) { (void)hipFree(d_in); return GZ_E_HIP; }
  if (hipMemcpy(d_in, blocks, (size_t)n * 128, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d_in); (void)hipFree(d_out); return GZ_E_HIP; }
  GZ_LAUNCH(k_idct_blocks, dim3(gz_div_up(n, kBlocksPerWG)), dim3(256), (hipStream_t)0, d_in, n, d_out);
  int rc = hipGetLastError() == hipSuccess ? GZ_OK : GZ_E_HIP;
  if (hipMemcpy(out, d_out, (size_t)n * 64, hipMemcpyDeviceToHost) != hipSuccess) rc = GZ_E_HIP;
  (void)hipFree(d_in); (void)hipFree(d_out);
  return rc;
}

int gz_probe_fdct_blocks(int device, int16_t* blocks, int n) {
  if (!blocks || n <= 0) return GZ_E_ARG;
  if (probe_device(device) != GZ_OK) return GZ_E_NO_DEVICE;
  int16_t* d = nullptr;
  if (hipMalloc((void**)&d, (size_t)n * 128) != hipSuccess) return GZ_E_HIP;
  if (hipMemcpy(d, blocks, (size_t)n * 128, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d); return GZ_E_HIP; }
  GZ_LAUNCH(k_fdct_blocks, dim3(gz_div_up(n, kBlocksPerWG)), dim3(256), (hipStream_t)0, d, n);
  int rc = hipGetLastError() == hipSuccess ? GZ_OK : GZ_E_HIP;
  if (hipMemcpy(blocks, d, (size_t)n * 128, hipMemcpyDeviceToHost) != hipSuccess) rc = GZ_E_HIP;
  (void)hipFree(d);
  return rc;
}


int gz_probe_rank_sort(int device, const float* keys, const int32_t* cnt, int narr, uint8_t* perm) {
  if (!keys || !cnt || !perm || narr <= 0) return GZ_E_ARG;
  for (int i = 0; i < narr; ++i) if (cnt[i] < 0 || cnt[i] > 192) return GZ_E_ARG;
  if (probe_device(device) != GZ_OK) return GZ_E_NO_DEVICE;
  DevBuf dk, dc, dp;
  if (!dk.alloc(sizeof(float) * narr * 192) || !dc.alloc(sizeof(int32_t) * narr) || !dp.alloc((size_t)narr * 192))
    return GZ_E_NOMEM;
  if (hipMemcpy(dk.p, keys, sizeof(float) * narr * 192, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dc.p, cnt, sizeof(int32_t) * narr, hipMemcpyHostToDevice) != hipSuccess)
    return GZ_E_HIP;
  const float* pk = (const float*)dk.p; const int32_t* pc = (const int32_t*)dc.p; uint8_t* pp = (uint8_t*)dp.p;
  GZ_LAUNCH(k_probe_rank_sort, dim3(gz_div_up(narr, kRankLanes)), dim3(kRankLanes), (hipStream_t)0, pk, pc, narr, pp);
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return GZ_E_HIP;
  if (hipMemcpy(perm, dp.p, (size_t)narr * 192, hipMemcpyDeviceToHost) != hipSuccess) return GZ_E_HIP;
  return GZ_OK;
}

int gz_probe_arith(int device, int op, const void* a, const void* b, const void* c,
                   void* out, int n) {
  if (!a || !out || n <= 0 || op < 0 || op > 6) return GZ_E_ARG;
  if (probe_device(device) != GZ_OK) return GZ_E_NO_DEVICE;
  const size_t es = (op == 2 || op == 3 || op == 5 || op == 6) ? 8 : 4;
  const size_t os = (op == 2 || op == 3 || op == 5) ? 8 : 4;
  void *da = nullptr, *db = nullptr, *dc = nullptr, *dout = nullptr;
  bool ok = hipMalloc(&da, es * n) == hipSuccess && hipMalloc(&db, es * n) == hipSuccess &&
            hipMalloc(&dc, es * n) == hipSuccess && hipMalloc(&dout, os * n) == hipSuccess;
  ok = ok && hipMemcpy(da, a, es * n, hipMemcpyHostToDevice) == hipSuccess;
  if (ok && b) ok = hipMemcpy(db, b, es * n, hipMemcpyHostToDevice) == hipSuccess;
  if (ok && c) ok = hipMemcpy(dc, c, es * n, hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) {
    (void)hipFree(da); (void)hipFree(db); (void)hipFree(dc); (void)hipFree(dout);
    return GZ_E_HIP;
  }
  GZ_LAUNCH(k_probe_arith, dim3(gz_div_up(n, 256)), dim3(256), (hipStream_t)0, op,
            (const void*)da, (const void*)db, (const void*)dc, dout, n);
  int rc = hipGetLastError() == hipSuccess ? GZ_OK : GZ_E_HIP;
  if (hipMemcpy(out, dout, os * n, hipMemcpyDeviceToHost) != hipSuccess) rc = GZ_E_HIP;
  (void)hipFree(da); (void)hipFree(db); (void)hipFree(dc); (void)hipFree(dout);
  return rc;
}

int gz_probe_math(int device, int op, int n, const void* a, const void* b, const void* c,
                  const double* p, int np, void* out) {
  if (!a || !out || n <= 0 || op < 0 || op >= GZ_MATH_OP_COUNT || np < 0 || (np > 0 && !p)) return GZ_E_ARG;
  // per op: number of input arrays, elements per input (in units of n), constants, outputs per element
  static const struct { int nin, per_in, np, outs; } kOps[GZ_MATH_OP_COUNT] = {
      {3, 1, 0, 2},    // GZ_MATH_DIV2_SHARED
      {2, 1, 4, 1},    // GZ_MATH_MALTA_DIFF
      {2, 1, 4, 1},    // GZ_MATH_MALTA_DIFF_PLAIN
      {1, 1, 0, 1},    // GZ_MATH_GAMMA_POLY
      {2, 3, 0, 3},    // GZ_MATH_OPSIN_PIXEL
      {1, 1, 1, 1},    // GZ_MATH_MAXIMUM_CLAMP
      {1, 1, 1, 1},    // GZ_MATH_REMOVE_RANGE
      {1, 1, 1, 1},    // GZ_MATH_AMPLIFY_RANGE
      {2, 1, 0, 1},    // GZ_MATH_SUPPRESS_X_BY_Y
      {2, 1, 2, 1},    // GZ_MATH_SUPPRESS_BRIGHT
      {3, 1, 0, 3},    // GZ_MATH_LF_TO_VALS
      {3, 1, 1, 1},    // GZ_MATH_L2DIFF
      {3, 1, 2, 1},    // GZ_MATH_L2DIFF_ASYM
      {2, 1, 0, 1},    // GZ_MATH_SAME_NOISE_PRE
      {2, 1, 0, 1},    // GZ_MATH_DIFF_FROM_SUPS
      {1, 1, 512, 1},  // GZ_MATH_INTERP_LUT512 (a, out: double)
      {2, 1, 0, 1},    // GZ_MATH_QUANT_DIV (a, b, out: int32)
      {1, 1, 2, 3},    // GZ_MATH_POW_TO_FLOAT (a, out: double)
  };
  const auto& o = kOps[op];
  if (np != o.np || (o.nin >= 2 && !b) || (o.nin >= 3 && !c)) return GZ_E_ARG;
  if (probe_device(device) != GZ_OK) return GZ_E_NO_DEVICE;
  const size_t es = op == GZ_MATH_INTERP_LUT512 || op == GZ_MATH_POW_TO_FLOAT ? 8 : 4;
  const size_t in_bytes = es * (size_t)o.per_in * n, out_bytes = es * (size_t)o.outs * n;
  DevBuf da, db, dc, dp, dout;
  if (!da.alloc(in_bytes) || !db.alloc(in_bytes) || !dc.alloc(in_bytes) || !dp.alloc(sizeof(double) * 512) ||
      !dout.alloc(out_bytes))
    return GZ_E_NOMEM;
  const void* src[3] = {a, b, c};
  void* dst[3] = {da.p, db.p, dc.p};
  for (int k = 0; k < o.nin; ++k)
    if (hipMemcpy(dst[k], src[k], in_bytes, hipMemcpyHostToDevice) != hipSuccess) return GZ_E_HIP;
  if (op == GZ_MATH_INTERP_LUT512 && hipMemcpy(dp.p, p, sizeof(double) * 512, hipMemcpyHostToDevice) != hipSuccess)
    return GZ_E_HIP;
  const dim3 grid(gz_div_up(n, 256));
  if (op == GZ_MATH_QUANT_DIV) {
    const int* pa = (const int*)da.p; const int* pq = (const int*)db.p; int* po = (int*)dout.p;
    GZ_LAUNCH(k_probe_quant_div, grid, dim3(256), (hipStream_t)0, pa, pq, po, n);
  } else if (op == GZ_MATH_POW_TO_FLOAT) {
    const double* pa = (const double*)da.p; double* po = (double*)dout.p;
    GZ_LAUNCH(k_probe_pow, grid, dim3(256), (hipStream_t)0, pa, n, p[0], p[1], kPowGuard, po);
  } else {
    ProbeMathArgs g;
    memset(&g, 0, sizeof(g));
    g.op = op; g.n = n;
    g.a = da.p; g.b = db.p; g.c = dc.p;
    g.table = (const double*)dp.p;
    g.out = dout.p;
    if (op == GZ_MATH_MALTA_DIFF || op == GZ_MATH_MALTA_DIFF_PLAIN) {
      g.nm.norm2_0gt1 = (float)p[0]; g.nm.norm2_0lt1 = (float)p[1]; g.nm.norm1f = (float)p[2];
      g.nm.fast_div = p[3] != 0.0 ? 1 : 0;
    } else if (op != GZ_MATH_INTERP_LUT512) {
      if (np > 0) g.p0 = p[0];
      if (np > 1) g.p1 = p[1];
    }
    GZ_LAUNCH(k_probe_math, grid, dim3(256), (hipStream_t)0, g);
  }
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return GZ_E_HIP;
  if (hipMemcpy(out, dout.p, out_bytes, hipMemcpyDeviceToHost) != hipSuccess) return GZ_E_HIP;
  return GZ_OK;
}

int gz_probe_div2_sweep(int device, const float* numerators, int nnum, unsigned stride, unsigned sample_every,
                        uint64_t* mismatches, float* sample, size_t sample_cap) {
  if (!numerators || !mismatches || nnum < 2 || nnum > 12 || (nnum & 1) || stride == 0 || sample_every == 0)
    return GZ_E_ARG;
  const unsigned long long total = 80ull << 23;                        // float denominators in [2^-40, 2^40)
  const unsigned long long count = (total + stride - 1) / stride;     // checked ones
  const unsigned long long nsample = (count + sample_every - 1) / sample_every;
  if (sample && sample_cap < nsample * (size_t)nnum) return GZ_E_ARG;
  if (probe_device(device) != GZ_OK) return GZ_E_NO_DEVICE;
  DevBuf dbad, dsample;
  if (!dbad.alloc(8) || (sample && !dsample.alloc(sizeof(float) * nsample * nnum))) return GZ_E_NOMEM;
  if (hipMemset(dbad.p, 0, 8) != hipSuccess) return GZ_E_HIP;
  Div2Numerators num;
  memset(&num, 0, sizeof(num));
  for (int k = 0; k < nnum; ++k) num.v[k] = numerators[k];
  unsigned long long* pbad = (unsigned long long*)dbad.p;
  float* psample = sample ? (float*)dsample.p : nullptr;
  GZ_LAUNCH(k_probe_div2_sweep, dim3((unsigned)((count + 255) / 256)), dim3(256), (hipStream_t)0, num, nnum, stride,
            count, sample_every, pbad, psample);
  if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return GZ_E_HIP;
  unsigned long long bad = 0;
  if (hipMemcpy(&bad, dbad.p, 8, hipMemcpyDeviceToHost) != hipSuccess) return GZ_E_HIP;
  if (sample && hipMemcpy(sample, dsample.p, sizeof(float) * nsample * nnum, hipMemcpyDeviceToHost) != hipSuccess)
    return GZ_E_HIP;
  *mismatches = bad;
  return GZ_OK;
}

// RGBToYUV420 (preprocess_downsample.cc:452-476) of a packed sRGB image by the device path of gz_downsample_silver,
// without a context: the three w x h planes it returns.
int gz_probe_silver_yuv420(int device, const uint8_t* srgb, int w, int h, int guard_log2, float* y, float* u, float* v,
                           uint64_t counters[2]) {
  if (!srgb || !y || !u || !v || w <= 0 || h <= 0 || w >= (1 << 16) || h >= (1 << 16) || (size_t)w * h > ((size_t)1 << 30) ||
      guard_log2 < -1 || guard_log2 > 64)
    return GZ_E_ARG;
  if (probe_device(device) != GZ_OK) return GZ_E_NO_DEVICE;
  const int w2 = (w + 1) / 2, h2 = (h + 1) / 2;
  const size_t n = (size_t)w * h, cells = (size_t)w2 * h2;
  struct HostBuf {   // scoped pinned allocation
    void* p = nullptr;
    ~HostBuf() { if (p) (void)hipHostFree(p); }
  } stage;
  DevBuf drgb, dlut, dplanes, dquarter, dlist;
  // four full planes (y_target, guess_y, out_u, out_v), six quarter planes (targets, the guesses' two halves)
  if (!drgb.alloc(3 * n) || !dlut.alloc(sizeof(float) * 256) || !dplanes.alloc(sizeof(float) * 4 * n) ||
      !dquarter.alloc(sizeof(float) * 6 * cells) || !dlist.alloc(sizeof(unsigned) * (cells + 1)) ||
      hipHostMalloc(&stage.p, kSilverStageBytes, kHostAllocFlags) != hipSuccess) {
    (void)hipGetLastError();
    return GZ_E_NOMEM;
  }
  if (hipMemcpy(drgb.p, srgb, 3 * n, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dlut.p, silver_lut(), sizeof(float) * 256, hipMemcpyHostToDevice) != hipSuccess)
    return GZ_E_HIP;
  float* planes = (float*)dplanes.p;
  float* quarter = (float*)dquarter.p;
  SilverRun r;
  r.stream = (hipStream_t)0;
  r.a.w = w; r.a.h = h; r.a.w2 = w2; r.a.h2 = h2;
  r.a.rgb = (const uint8_t*)drgb.p;
  r.a.lut = (const float*)dlut.p;
  r.a.y_target = planes; r.a.guess_y = planes + n; r.out_u = planes + 2 * n; r.out_v = planes + 3 * n;
  r.a.target_u = quarter; r.a.target_v = quarter + cells;
  r.a.guess_u[0] = quarter + 2 * cells; r.a.guess_v[0] = quarter + 3 * cells;
  r.a.guess_u[1] = quarter + 4 * cells; r.a.guess_v[1] = quarter + 5 * cells;
  r.a.list = (unsigned*)dlist.p;
  r.a.guard = guard_log2 == 64 ? 0.0 : guard_log2 < 0 ? kPowGuard : ldexp(1.0, -guard_log2);
  r.a.list_all = guard_log2 < 0 ? 1 : 0;
  r.stage = (float*)stage.p;
  std::string err;
  if (const int rc = silver_run(r, counters, &err)) return rc;
  if (hipDeviceSynchronize() != hipSuccess) return GZ_E_HIP;
  if (hipMemcpy(y, r.a.guess_y, sizeof(float) * n, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(u, r.out_u, sizeof(float) * n, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(v, r.out_v, sizeof(float) * n, hipMemcpyDeviceToHost) != hipSuccess)
    return GZ_E_HIP;
  return GZ_OK;
}

// k_scan_offsets alone, without a context: one scratch sized for the largest of `lengths`, one launch per entry on the
// first lengths[i] of `values`, back to back on one stream, the epochs following start_epoch by the rule
// enqueue_scan_offsets follows (scan_next_epoch) -- nothing else clears the scratch between the launches.
// out: every launch's off[0 .. lengths[i]], one after the other.
int gz_probe_scan_offsets(int device, const uint32_t* values, int n_values, const int32_t* lengths, int n_lengths,
                          uint32_t start_epoch, uint64_t* out) {
  if (!values || !lengths || !out || n_values <= 0 || n_lengths <= 0 || n_lengths > 4096 || start_epoch >= 0x3fffffffu)
    return GZ_E_ARG;
  int max_len = 0;
  size_t total = 0;
  for (int i = 0; i < n_lengths; ++i) {
    if (lengths[i] <= 0 || lengths[i] > n_values) return GZ_E_ARG;
    max_len = std::max(max_len, (int)lengths[i]);
    total += (size_t)lengths[i] + 1;
  }
  if (total > ((size_t)1 << 28)) return GZ_E_ARG;
  if (probe_device(device) != GZ_OK) return GZ_E_NO_DEVICE;
  const int max_tiles = gz_div_up(max_len, kScanTile) + 1;
  const size_t bytes = scan_state_bytes(max_tiles);
  DevBuf dv, dstate, doff;
  if (!dv.alloc(sizeof(uint32_t) * n_values) || !dstate.alloc(bytes) || !doff.alloc(sizeof(unsigned long long) * total))
    return GZ_E_NOMEM;
  const hipStream_t stream = (hipStream_t)0;
  if (hipMemcpy(dv.p, values, sizeof(uint32_t) * n_values, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemsetAsync(dstate.p, 0, bytes, stream) != hipSuccess)
    return GZ_E_HIP;
  const ScanState st = scan_state_at(dstate.p, max_tiles);
  const unsigned* bits = (const unsigned*)dv.p;
  unsigned long long* off = (unsigned long long*)doff.p;
  unsigned epoch = start_epoch;
  for (int i = 0; i < n_lengths; ++i) {
    if (scan_next_epoch(&epoch, dstate.p, bytes, stream) != hipSuccess) return GZ_E_HIP;
    const int n = lengths[i];
    GZ_LAUNCH(k_scan_offsets, dim3(gz_div_up(n, kScanTile)), dim3(256), stream, bits, n, off, st, epoch);
    if (hipGetLastError() != hipSuccess) return GZ_E_HIP;
    off += (size_t)n + 1;
  }
  if (hipStreamSynchronize(stream) != hipSuccess) return GZ_E_HIP;
  if (hipMemcpy(out, doff.p, sizeof(unsigned long long) * total, hipMemcpyDeviceToHost) != hipSuccess) return GZ_E_HIP;
  return GZ_OK;
}

// ---- phase B on state the tests choose (tests/order_domain.py): the hooks put block maxima and candidates where a
// gz_compare and a block search leave them, and read the device's weights and max_block_error back; they launch no
// kernel of their own, everything under test runs through the production entry points.
int gz_probe_set_block_max(gz_ctx* c, const float* block_max) {
  DeviceScope ds_(c);
  if (!c || !block_max) return GZ_E_ARG;
  c->have_distmap = c->h_block_max_valid = false;
  HIPCHK(c, hipMemcpyAsync(c->d_block_max, block_max, sizeof(float) * c->nb, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->have_distmap = true;
  return GZ_OK;
}

int gz_probe_set_search(gz_ctx* c, int comp_mask, const int32_t* offsets, const uint8_t* idx, const float* err) {
  DeviceScope ds_(c);
  if (!c || !offsets || !idx || !err || comp_mask < 1 || comp_mask > 7) return GZ_E_ARG;
  int mode = 0;
  TRY(search_mode_of(c, comp_mask, &mode));
  const int gn = mode == 2 ? c->nbc : c->nb;
  if (offsets[0] != 0) return GZ_E_ARG;
  for (int b = 0; b < gn; ++b)
    if (offsets[b + 1] < offsets[b] || offsets[b + 1] - offsets[b] > 192) return GZ_E_ARG;
  TRY(search_grid_begin(c, comp_mask, mode));
  // k_block_search's layout: a count per block, its indices and errors at a stride of 192
  std::vector<int32_t> cnt(gn);
  std::vector<uint8_t> widx((size_t)gn * 192, 0);
  std::vector<float> werr((size_t)gn * 192, 0.0f);
  for (int b = 0; b < gn; ++b) {
    cnt[b] = offsets[b + 1] - offsets[b];
    memcpy(widx.data() + (size_t)b * 192, idx + offsets[b], (size_t)cnt[b]);
    memcpy(werr.data() + (size_t)b * 192, err + offsets[b], sizeof(float) * (size_t)cnt[b]);
  }
  HIPCHK(c, hipMemcpyAsync(c->d_out_cnt, cnt.data(), sizeof(int32_t) * gn, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_out_idx, widx.data(), (size_t)gn * 192, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_out_err, werr.data(), sizeof(float) * gn * 192, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  search_installed(c, (size_t)offsets[gn]);
  return GZ_OK;
}

int gz_probe_order_state(gz_ctx* c, float* weight, float* max_err) {
  DeviceScope ds_(c);
  if (!c) return GZ_E_ARG;
  if (!c->have_search || !c->made.order_blocks) { c->err = "gz_order_build* must precede gz_probe_order_state"; return GZ_E_STATE; }
  TRY(flush_order_advance(c));
  const size_t bytes = sizeof(float) * (size_t)c->sg_n;
  if (weight) HIPCHK(c, hipMemcpyAsync(weight, c->d_weight, bytes, hipMemcpyDeviceToHost, c->stream));
  if (max_err) HIPCHK(c, hipMemcpyAsync(max_err, c->d_max_err, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return GZ_OK;
}

#ifdef GZ_EMU
// Emulation build only: the emulated device pow of gz_pow_to_float_guarded off by u double ulps (the device library's
// pow is accurate to a few ulps, and not libm's: in the emulation it IS libm's, and the guard would have nothing to catch)
__attribute__((used, visibility("default"))) void gz_emu_set_pow_ulps(int u) { gz::gz_emu_pow_ulps() = u; }
// Emulation build only (test hook, in the style of gz_emu_fail_launch): the emulated reciprocal of
// div2_shared off by u = -1, 0, +1 ulp -- v_rcp_f32 is accurate to 1 ulp, not correctly rounded.
__attribute__((used, visibility("default"))) void gz_emu_set_rcp_ulps(int u) { gz::gz_emu_rcp_ulps() = u; }
#endif

#endif  // GZ_NO_PROBES

}  // extern "C"
