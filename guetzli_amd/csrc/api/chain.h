// The Compare chain: blur dispatch (which instantiation for which size), the stream graph (ChainStreams, fork), the pipeline stages (opsin, SeparateFrequencies, mask branch, Malta, combine, final blur) on three streams, reconstruction, the chain's self-checks, the block mask.
// (part of the one translation unit gz_api.hip, which includes these files in order; split by
// concern in round 5 -- no declaration here is visible outside libguetzli_amd.so but the C ABI)
#pragma once

namespace {
// ------------------------------------------------------------- blur dispatch helpers --
// Radius < 16: one fused launch per blur (k_blur2d); radius >= 16: a row pass and a column pass.
// Two measured crossovers pick the instantiation (both can be forced through the context's gz_config --
// from GZ_BLUR_PK / GZ_TILE_ROWS at gz_create -- so that the tests run every one of them on images small enough
// for the emulation):
//  * blur_packed -- row-pair / column-pair passes with packed arithmetic (k_blur_h_pk, k_blur_v_pk:
//    twice the outputs per thread, half the LDS reads and address computations per output, half
//    the workgroups) from 1.5 MPix on (round 5; 4 MPix until then), the one-output-row kernels (k_blur_h, k_blur_v_compact) below
//    (profiles/r02_packed_blur_ab.log, r03_chain_kernel_experiments.log);
//  * tile_rows -- 64 x 32 tiles from 7 MPix on, 64 x 16 below: twice the workgroups for
//    256 CUs (720p: 0.290 -> 0.257 ms per Compare; round 5: 1080p 0.343 -> 0.330, equal at 4K).
// What round 4 removed after it had lost every A/B of rounds 2 and 3: the unrolled (non-compact)
// column pass and fused kernels, 64-row tiles, the epilogue without 16-byte accesses and the row
// pass with LDS bank conflicts (GZ_BLUR_OPT), the three-plane LF passes, the unpaired mask blurs.
// Every dispatcher and stage below launches on the stream it is given.
// A batched chain (c->batch.n > 0, entry_batch.h) has ONE configuration, whatever the context's gz_config says: the
// unpacked passes and 16-row tiles everywhere -- what an image under 1.5 MPix gets by default.
static bool packed_blur(const gz_ctx* c) {
  if (c->batch.n) return false;
  if (c->cfg.blur_packed >= 0) return c->cfg.blur_packed != 0;
  // (round 5, with 16-row tiles: 1080p 0.3356 -> 0.3290 ms, 2560 x 1440 0.487 -> 0.466, 3200 x 1800 0.719 -> 0.684;
  // 720p equal -- profiles/r05_chain_experiments.log, section 8)
  return (size_t)c->w * c->h >= 1500000;
}
constexpr int kTileRows = 32;
constexpr int kSmallTileRows = 16;
static bool small_tiles(const gz_ctx* c) {
  if (c->batch.n) return true;
  if (c->cfg.tile_rows == 16) return true;
  if (c->cfg.tile_rows == 32) return false;
  // (round 5: 16-row tiles win or tie up to 3200 x 1800 -- 1080p chain 0.343 -> 0.330 ms, sixteen 1080p images
  // four in flight 27.7 -> 29.5 MPix/s; equal at 3840 x 2160: profiles/r05_chain_experiments.log, section 8)
  return (size_t)c->w * c->h < 7000000;
}

// PAIR (with `second`): two blurs of equal radius and different sigma on two independent planes as ONE launch per
// pass (grid z = plane; plane 1 takes the second tap set): the mask's radius-20 pair (butteraugli.cc:1780-1790).
// MAYBATCH (all three dispatchers): the Compare chain's calls, which a batched chain makes too -- c->batch.n images per
// launch, the image index in the grid's z (gz_common.h, BatchIdx).  false (blur_plane: the probes) carries no batched
// instantiation.
static int no_batched_form(gz_ctx* c) { c->err = "this launch has no batched form"; return GZ_E_STATE; }
template <int R, class Src, int NC, bool PAIR = false, bool MAYBATCH = true>
int blur_h(gz_ctx* c, hipStream_t stream, const SrcPack<Src, NC>& src, const PlanePack<NC>& dst,
           const BlurCfg& cfg, const BlurCfg* second = nullptr) {
  if (PAIR != (second != nullptr)) { c->err = "blur pair mismatch"; return GZ_E_STATE; }
  if (!MAYBATCH && c->batch.n) return no_batched_form(c);
  const BlurCfg& cfg1 = PAIR ? *second : cfg;
  if (cfg.r != R || cfg1.r != R) { c->err = "blur radius mismatch"; return GZ_E_STATE; }
  const Taps<R> t0 = taps_of<R>(cfg), t1 = taps_of<R>(cfg1);
  const BorderScale b0 = cfg.bx, b1 = cfg1.bx;
  const int w = c->w, h = c->h, pitch = c->pitch;
  if (packed_blur(c)) {
    dim3 grid(gz_div_up(c->w, HW), gz_div_up(c->h, HP), NC);
    GZ_LAUNCH((k_blur_h_pk<R, Src, NC, PAIR>), grid, dim3(256), stream, src, dst, w, h, pitch, t0, b0, t1, b1);
  } else {
    dim3 grid(gz_div_up(c->w, HW), gz_div_up(c->h, HH), NC);
    if constexpr (MAYBATCH) {
      if (c->batch.n) {
        grid.z *= c->batch.n;
        const BatchIdx bi = c->batch.idx;
        GZ_LAUNCH((k_blur_h<R, Src, NC, PAIR, BatchIdx>), grid, dim3(256), stream, src, dst, w, h, pitch, t0, b0, t1, b1, bi);
        KCHK(c);
        return GZ_OK;
      }
    }
    GZ_LAUNCH((k_blur_h<R, Src, NC, PAIR>), grid, dim3(256), stream, src, dst, w, h, pitch, t0, b0, t1, b1);
  }
  KCHK(c);
  return GZ_OK;
}

template <int R, int NC, class Post, bool PAIR = false, bool MAYBATCH = true>
int blur_v(gz_ctx* c, hipStream_t stream, const CPlanePack<NC>& src, const Post& post, const BlurCfg& cfg,
           const BlurCfg* second = nullptr) {
  if (PAIR != (second != nullptr)) { c->err = "blur pair mismatch"; return GZ_E_STATE; }
  if (!MAYBATCH && c->batch.n) return no_batched_form(c);
  const BlurCfg& cfg1 = PAIR ? *second : cfg;
  if (cfg.r != R || cfg1.r != R) { c->err = "blur radius mismatch"; return GZ_E_STATE; }
  const Taps<R> t0 = taps_of<R>(cfg), t1 = taps_of<R>(cfg1);
  const BorderScale b0 = cfg.by, b1 = cfg1.by;
  const int w = c->w, h = c->h, pitch = c->pitch;
  const bool small = small_tiles(c);
  dim3 grid(gz_div_up(c->w, VW), gz_div_up(c->h, small ? kSmallTileRows : kTileRows), PAIR ? 2 : 1);
  if constexpr (MAYBATCH) {
    if (c->batch.n) {   // (unpacked, 16-row tiles: packed_blur, small_tiles)
      grid.z *= c->batch.n;
      const BatchIdx bi = c->batch.idx;
      GZ_LAUNCH((k_blur_v_compact<R, NC, Post, kSmallTileRows, PAIR, BatchIdx>), grid, dim3(256), stream, src, post, w, h, pitch, t0, b0, t1, b1, bi);
      KCHK(c);
      return GZ_OK;
    }
  }
  if (packed_blur(c)) {
    if (small) GZ_LAUNCH((k_blur_v_pk<R, NC, Post, kSmallTileRows, PAIR>), grid, dim3(256), stream, src, post, w, h, pitch, t0, b0, t1, b1);
    else GZ_LAUNCH((k_blur_v_pk<R, NC, Post, kTileRows, PAIR>), grid, dim3(256), stream, src, post, w, h, pitch, t0, b0, t1, b1);
  } else {
    if (small) GZ_LAUNCH((k_blur_v_compact<R, NC, Post, kSmallTileRows, PAIR>), grid, dim3(256), stream, src, post, w, h, pitch, t0, b0, t1, b1);
    else GZ_LAUNCH((k_blur_v_compact<R, NC, Post, kTileRows, PAIR>), grid, dim3(256), stream, src, post, w, h, pitch, t0, b0, t1, b1);
  }
  KCHK(c);
  return GZ_OK;
}

// BM = true (the chain's last blur): the Post functor's results are also reduced to the per-block
// maxima and the image maximum; that kernel keeps its results in registers (always 32-row tiles).
// bm.tiles + n_tiles: the listed tiles only (tile ids of the grid this function would launch).
// A batched launch: no tile list and no block maxima; bm.image_max_bits is the first of c->batch.n words, one per image.
template <int R, int NC, class Src, class Post, bool BM = false, bool MAYBATCH = true>
int blur2d(gz_ctx* c, hipStream_t stream, const SrcPack<Src, NC>& src, const Post& post, const BlurCfg& cfg,
           BlockMaxOut bm = BlockMaxOut{nullptr, nullptr, 0, nullptr}, int n_tiles = 0) {
  if (cfg.r != R) { c->err = "blur radius mismatch"; return GZ_E_STATE; }
  if (c->batch.n && (!MAYBATCH || bm.tiles || bm.block_max)) return no_batched_form(c);
  const Taps<R> tp = taps_of<R>(cfg);
  const BorderScale bx = cfg.bx, by = cfg.by;
  const int w = c->w, h = c->h, pitch = c->pitch;
  // (the chain's last blur, with block maxima: 16-row tiles below 1.5 MPix only -- 720p chain 0.224 -> 0.213 ms,
  // nothing at 1080p, +3 % at 2560 x 1440: profiles/r05_chain_experiments.log, section 8)
  // (a tile list: always the 16-row tiles -- a handful of workgroups, whose time is one workgroup's latency)
  const bool small = bm.tiles || (BM ? small_tiles(c) && (size_t)c->w * c->h < 1500000 : small_tiles(c));
  const dim3 grid = bm.tiles ? dim3(n_tiles) : dim3(gz_div_up(c->w, T2), gz_div_up(c->h, small ? kSmallTileRows : kTileRows));
  if constexpr (MAYBATCH) {
    if (c->batch.n) {   // (16-row tiles, the last blur included: small_tiles, and a batch's images are under 1.5 MPix)
      const dim3 bgrid(grid.x, grid.y, c->batch.n);
      const BatchIdx bi = c->batch.idx;
      GZ_LAUNCH((k_blur2d<R, NC, Src, Post, BM, kSmallTileRows, BatchIdx>), bgrid, dim3(256), stream, src, post, w, h, pitch, tp, bx, by, bm, bi);
      KCHK(c);
      return GZ_OK;
    }
  }
  if (small) GZ_LAUNCH((k_blur2d<R, NC, Src, Post, BM, kSmallTileRows>), grid, dim3(256), stream, src, post, w, h, pitch, tp, bx, by, bm);
  else GZ_LAUNCH((k_blur2d<R, NC, Src, Post, BM, kTileRows>), grid, dim3(256), stream, src, post, w, h, pitch, tp, bx, by, bm);
  KCHK(c);
  return GZ_OK;
}

#define TRY(x) do { int rc_ = (x); if (rc_ != GZ_OK) return rc_; } while (0)

// One plane blurred with any of the chain's radii, by the kernels gz_compare uses for that radius: fused below 16,
// two passes (through `tmp`) from 16 up.  A template on the Post functor, instantiated where it is used (gz_probe_blur):
// a build without the probes (GZ_NO_PROBES) does not carry the instantiations that only they launch.
template <int R, class Post>
int blur_plane_r(gz_ctx* c, hipStream_t stream, const SrcPack<SrcPlain, 1>& src, float* tmp, const Post& post, const BlurCfg& cfg) {
  if constexpr (R < 16) {
    return blur2d<R, 1, SrcPlain, Post, false, false>(c, stream, src, post, cfg);
  } else {
    PlanePack<1> t; CPlanePack<1> ct;
    t.p[0] = tmp; ct.p[0] = tmp;
    TRY((blur_h<R, SrcPlain, 1, false, false>(c, stream, src, t, cfg)));
    return blur_v<R, 1, Post, false, false>(c, stream, ct, post, cfg);
  }
}
template <class Post>
int blur_plane(gz_ctx* c, hipStream_t stream, const SrcPack<SrcPlain, 1>& src, float* tmp, const Post& post, const BlurCfg& cfg) {
  switch (cfg.r) {
    case 2: return blur_plane_r<2>(c, stream, src, tmp, post, cfg);
    case 3: return blur_plane_r<3>(c, stream, src, tmp, post, cfg);
    case 4: return blur_plane_r<4>(c, stream, src, tmp, post, cfg);
    case 5: return blur_plane_r<5>(c, stream, src, tmp, post, cfg);
    case 8: return blur_plane_r<8>(c, stream, src, tmp, post, cfg);
    case 16: return blur_plane_r<16>(c, stream, src, tmp, post, cfg);
    case 20: return blur_plane_r<20>(c, stream, src, tmp, post, cfg);
    case 23: return blur_plane_r<23>(c, stream, src, tmp, post, cfg);
  }
  c->err = "unsupported blur radius";
  return GZ_E_ARG;
}

// ctx_owns: cfg is a member of the context, whose record takes the scales; a local cfg's block is its caller's to free.
int setup_blur_cfg(gz_ctx* c, BlurCfg* cfg, float sigma, float border_ratio, bool ctx_owns) {
  make_taps_host(sigma, cfg);
  cfg->border_ratio = border_ratio;
  std::vector<float> xl, xh, yl, yh;
  border_scales_host(*cfg, c->w, &xl, &xh);
  border_scales_host(*cfg, c->h, &yl, &yh);
  const int r = cfg->r;
  if (ctx_owns) TRY(regrow(c, nullptr, nullptr, 0, {{(void**)&cfg->d_scale, sizeof(float) * 4 * r}}));
  else HIPCHK(c, pool_malloc((void**)&cfg->d_scale, sizeof(float) * 4 * r));
  std::vector<float> all;
  all.insert(all.end(), xl.begin(), xl.end());
  all.insert(all.end(), xh.begin(), xh.end());
  all.insert(all.end(), yl.begin(), yl.end());
  all.insert(all.end(), yh.begin(), yh.end());
  HIPCHK(c, hipMemcpy(cfg->d_scale, all.data(), sizeof(float) * 4 * r, hipMemcpyHostToDevice));
  cfg->bx.lo = cfg->d_scale;
  cfg->bx.hi = cfg->d_scale + r;
  cfg->by.lo = cfg->d_scale + 2 * r;
  cfg->by.hi = cfg->d_scale + 3 * r;
  return GZ_OK;
}

// ------------------------------------------------------------------ the stream graph --
// The SameNoise blur and the mask branch (DiffPrecompute + three blurs; scratch planes
// tmp[0..2], snb, diffx, diffy, mxb, myb1, myb2) read only the two PsychoImages, so they run
// on the side stream while the main stream does Malta; k_combine needs both.  At 1080p a launch is
// ~1000 workgroups for 256 CUs and the kernels are latency-bound: the overlap is worth ~10 %.
// cfg.single_stream: 1 = the whole Compare on the main stream (per-kernel profiling; no fork / join events),
// 0 = the three-stream chain, -1 (default) = by company: three streams for a context that has the device to itself,
// ONE when other contexts are alive on it (a batch's images in flight).  The side streams buy a lone chain its
// overlap (1080p 0.326 against 0.371 ms); several images in flight overlap each other instead, and every fork /
// join costs host time in a runtime four threads are calling into: one stream per image is +65 % at 512 x 512,
// +12-25 % at 1 MPix, +10 % at 1080p, +4 % at 4K (profiles/r06_chain_experiments.log, section 6).  The choice is
// made per Compare and changes no result: every Compare joins its side streams before it ends.
static bool single_stream_wanted(const gz_ctx* c) {
  if (c->cfg.single_stream >= 0) return c->cfg.single_stream != 0;
  return slots_taken(c->device) > 1;
}
// ... decided ONCE per Compare (enqueue_compare) and handed to its stages as this value: contexts come and go on other
// threads while a Compare is being enqueued, and a fork made for three streams must not meet a join that thinks there
// was one.  Not forked: all three are the main stream, and the same code enqueues the same kernels in the same order.
struct ChainStreams {
  hipStream_t main, side, side2;
};
static ChainStreams chain_streams(const gz_ctx* c, bool forked) {
  return forked ? ChainStreams{c->stream, c->side_stream, c->side_stream2} : ChainStreams{c->stream, c->stream, c->stream};
}
// An edge of the graph: what `to` gets from here on runs behind what `from` holds now.  Recorded and waited for only
// when the two differ (a stream keeps its own order); fork() is both halves, a join records where its branch ends and
// waits where its results are needed.
static int record_for(gz_ctx* c, hipStream_t from, hipStream_t to, hipEvent_t ev) {
  if (from != to) HIPCHK(c, hipEventRecord(ev, from));
  return GZ_OK;
}
static int wait_for(gz_ctx* c, hipStream_t from, hipStream_t to, hipEvent_t ev) {
  if (from != to) HIPCHK(c, hipStreamWaitEvent(to, ev, 0));
  return GZ_OK;
}
static int fork(gz_ctx* c, hipStream_t from, hipStream_t to, hipEvent_t ev) {
  TRY(record_for(c, from, to, ev));
  return wait_for(c, from, to, ev);
}

// --------------------------------------------------------------- pipeline stages ------
// OpsinDynamicsImage: lin[3] -> xyb[3]
// tiles (optional): only the listed tiles of the launch's grid (opsin_tile_rows() high), n_tiles of them.
int stage_opsin(gz_ctx* c, hipStream_t stream, const int* tiles = nullptr, int n_tiles = 0) {
  SrcPack<SrcPlain, 3> s;
  for (int i = 0; i < 3; ++i) s.s[i].p = c->lin[i];
  PostOpsin post;
  for (int i = 0; i < 3; ++i) { post.lin[i] = c->lin[i]; post.xyb[i] = c->xyb[i]; }
  return blur2d<2, 3, SrcPlain, PostOpsin>(c, stream, s, post, c->blur[B_OPSIN], BlockMaxOut{nullptr, nullptr, 0, tiles}, n_tiles);
}
static int opsin_tile_rows(const gz_ctx*) { return kSmallTileRows; }   // (of a tile LIST: blur2d)

// SeparateFrequencies: xyb[3] -> Psycho planes
// The LF blur (radius 16) runs as X / Y (two planes, PostLFxy) and B (one plane, PostLFb: its
// XybLowFreqToVals mixes in the raw LF of Y the first wrote, butteraugli.cc:386-389).  B -- which only k_combine
// reads -- goes to cs.side2 (the candidate's chain, when forked), beside the MF / HF bands instead of in front of
// them; the caller joins that stream before k_combine (stage_diffmap).  Its row-pass result goes through the
// distance-map plane, which nothing else touches before the chain's last kernel.
int stage_separate(gz_ctx* c, const ChainStreams& cs, Psycho* ps) {
  c->have_map_plane = false;   // (the plane is written below: whatever map it held is gone)
  TRY(fork(c, cs.main, cs.side2, c->ev_xyb));
  {
    SrcPack<SrcPlain, 1> s; PlanePack<1> t;
    s.s[0].p = c->xyb[2]; t.p[0] = c->distmap;
    TRY((blur_h<16, SrcPlain, 1>(c, cs.side2, s, t, c->blur[B_LF])));
  }
  {
    SrcPack<SrcPlain, 2> s; PlanePack<2> t; CPlanePack<2> ct;
    for (int i = 0; i < 2; ++i) { s.s[i].p = c->xyb[i]; t.p[i] = c->tmp[i]; ct.p[i] = c->tmp[i]; }
    TRY((blur_h<16, SrcPlain, 2>(c, cs.main, s, t, c->blur[B_LF])));
    PostLFxy post;
    for (int i = 0; i < 2; ++i) { post.lf_raw[i] = c->lf_raw[i]; post.lf_vals[i] = ps->lfv[i]; }
    TRY((blur_v<16, 2, PostLFxy>(c, cs.main, ct, post, c->blur[B_LF])));
  }
  TRY(fork(c, cs.main, cs.side2, c->ev_lfy));
  {
    CPlanePack<1> ct; ct.p[0] = c->distmap;
    PostLFb post; post.lf_raw_y = c->lf_raw[1]; post.lf_vals_b = ps->lfv[2];
    TRY((blur_v<16, 1, PostLFb>(c, cs.side2, ct, post, c->blur[B_LF])));
  }
  {  // MF (X, Y)
    SrcPack<SrcDiff, 2> s;
    for (int i = 0; i < 2; ++i) {
      s.s[i].a = c->xyb[i];
      s.s[i].b = c->lf_raw[i];
    }
    PostMF post;
    for (int i = 0; i < 2; ++i) {
      post.xyb[i] = c->xyb[i];
      post.lf_raw[i] = c->lf_raw[i];
      post.mf[i] = ps->mf[i];
      post.hf_pre[i] = c->hfp[i];
    }
    TRY((blur2d<8, 2, SrcDiff, PostMF>(c, cs.main, s, post, c->blur[B_MF])));
  }
  {  // HF / UHF
    SrcPack<SrcPlain, 2> s;
    for (int i = 0; i < 2; ++i) s.s[i].p = c->hfp[i];
    PostHF post;
    for (int i = 0; i < 2; ++i) {
      post.hf_pre[i] = c->hfp[i];
      post.hf[i] = ps->hf[i];
      post.uhf[i] = ps->uhf[i];
    }
    post.lf_raw_y = c->lf_raw[1];
    TRY((blur2d<4, 2, SrcPlain, PostHF>(c, cs.main, s, post, c->blur[B_HF])));
  }
  return GZ_OK;
}

// Mask first half: DiffPrecompute + three blurs -> mxb, myb1, myb2, on `stream`.  The three blurs only share
// their input: the two of radius 20 (X: sigma r2 = 9.24; Y second: sigma r1 = 9.04 -- separate
// taps) are one launch per pass (grid z = plane); the small one (radius 5) goes to `small_stream`, behind
// whatever is queued there (the SameNoise blur, the shorter of the two side branches).
int stage_mask_blurs(gz_ctx* c, hipStream_t stream, hipStream_t small_stream, const MaskPrePack& pk) {
  dim3 grid(gz_div_up(c->w, 1024), c->h, 2);
  if (c->batch.n) {
    grid.z *= c->batch.n;
    GZ_LAUNCH((k_mask_pre<BatchIdx>), grid, dim3(256), stream, pk, c->w, c->h, c->pitch, c->batch.idx);
  } else {
    GZ_LAUNCH(k_mask_pre, grid, dim3(256), stream, pk, c->w, c->h, c->pitch);
  }
  KCHK(c);
  TRY(fork(c, stream, small_stream, c->ev_mask_pre));
  {
    SrcPack<SrcPlain, 2> s; PlanePack<2> t; CPlanePack<2> ct;
    s.s[0].p = c->diffx; s.s[1].p = c->diffy;
    t.p[0] = c->tmp[1]; t.p[1] = c->tmp[2];
    ct.p[0] = c->tmp[1]; ct.p[1] = c->tmp[2];
    TRY((blur_h<20, SrcPlain, 2, true>(c, stream, s, t, c->blur[B_MASKX], &c->blur[B_MASKY1])));
    PostStore<2> post; post.out[0] = c->mxb; post.out[1] = c->myb2;
    TRY((blur_v<20, 2, PostStore<2>, true>(c, stream, ct, post, c->blur[B_MASKX], &c->blur[B_MASKY1])));
  }
  {
    SrcPack<SrcPlain, 1> s; s.s[0].p = c->diffy;
    PostStore<1> post; post.out[0] = c->myb1;
    TRY((blur2d<5, 1, SrcPlain, PostStore<1>>(c, small_stream, s, post, c->blur[B_MASKY0])));
  }
  return GZ_OK;
}

// MaskPsychoImage's inputs (butteraugli.cc:753-782): a * uhf + b * hf of a PsychoImage, X and Y.
static void mask_in_psycho(const Psycho& p, MaskIn in[2]) {
  const double muls[4] = {0, 1.64178305129, 0.831081703362, 3.23680933546};   // (:759-764)
  for (int i = 0; i < 2; ++i) {
    in[i].a = muls[2 * i];
    in[i].b = muls[2 * i + 1];
    in[i].plain = 0;
    in[i].hf = p.hf[i];
    in[i].uhf = muls[2 * i] == 0 ? nullptr : p.uhf[i];
  }
}
// The original's half, once per image (gz_set_rgb): c->sup0.
int stage_mask_sup(gz_ctx* c, hipStream_t stream, const MaskIn in[2], float* const out[2]) {
  MaskSupPack pk;
  for (int i = 0; i < 2; ++i) { pk.in[i] = in[i]; pk.out[i] = out[i]; }
  dim3 grid(gz_div_up(c->w, 1024), c->h, 2);
  if (c->batch.n) {
    grid.z *= c->batch.n;
    GZ_LAUNCH((k_mask_sup<BatchIdx>), grid, dim3(256), stream, pk, c->w, c->h, c->pitch, c->batch.idx);
  } else {
    GZ_LAUNCH(k_mask_sup, grid, dim3(256), stream, pk, c->w, c->h, c->pitch);
  }
  KCHK(c);
  return GZ_OK;
}
MaskPrePack mask_pack_psycho(gz_ctx* c, const Psycho& b) {
  MaskPrePack pk;
  mask_in_psycho(b, pk.in1);
  pk.sup0[0] = c->sup0[0];
  pk.sup0[1] = c->sup0[1];
  pk.out[0] = c->diffx;
  pk.out[1] = c->diffy;
  return pk;
}
int ensure_pip(gz_ctx* c);
// Mask(xyb0, xyb1) on raw planes (StartBlockComparisons' mask of the original with itself, the
// stage probe): image 0's half goes through two scratch planes of the probe arena.
int mask_pack_plain(gz_ctx* c, hipStream_t stream, const float* const a[2], const float* const b[2], MaskPrePack* pk) {
  MaskIn in0[2];
  for (int i = 0; i < 2; ++i) {
    in0[i] = {nullptr, a[i], 0.0, 1.0, 1};
    pk->in1[i] = {nullptr, b[i], 0.0, 1.0, 1};
  }
  TRY(ensure_pip(c));   // (sup_scratch)
  TRY(stage_mask_sup(c, stream, in0, c->sup_scratch));
  pk->sup0[0] = c->sup_scratch[0];
  pk->sup0[1] = c->sup_scratch[1];
  pk->out[0] = c->diffx;
  pk->out[1] = c->diffy;
  return GZ_OK;
}

// k_combine's arguments for the mask alone (no diffmap): the three mask blurs in, mask planes (and, given, the DC
// mask planes) out.  stage_diffmap fills in the rest.
static CombineArgs combine_mask_args(const gz_ctx* c, float* const mask_out[3], float* const mask_dc_out[3]) {
  CombineArgs a;
  memset(&a, 0, sizeof(a));
  a.mask_x_blur = c->mxb; a.mask_y_blur1 = c->myb1; a.mask_y_blur2 = c->myb2;
  a.luts = c->d_mask_luts;
  for (int i = 0; i < 3; ++i) {
    a.mask_out[i] = mask_out ? mask_out[i] : nullptr;
    a.mask_dc_out[i] = mask_dc_out ? mask_dc_out[i] : nullptr;
  }
  return a;
}
static int launch_combine(gz_ctx* c, hipStream_t stream, const CombineArgs& a) {
  dim3 grid(gz_div_up(c->w, 1024), c->h);   // (4 pixels per thread)
  if (c->batch.n) {
    grid.z = c->batch.n;
    GZ_LAUNCH((k_combine<BatchIdx>), grid, dim3(256), stream, a, c->w, c->h, c->pitch, c->batch.idx);
  } else {
    GZ_LAUNCH(k_combine, grid, dim3(256), stream, a, c->w, c->h, c->pitch);
  }
  KCHK(c);
  return GZ_OK;
}

// The SameNoise blur (cs.side2) and the mask branch (cs.side, its radius-5 blur behind the SameNoise blur on
// cs.side2), forked off cs.main; both branches end in the events stage_diffmap waits for before k_combine.
int fork_side_branch(gz_ctx* c, const ChainStreams& cs, const Psycho& p0, const Psycho& p1) {
  TRY(fork(c, cs.main, cs.side, c->ev_fork));
  TRY(wait_for(c, cs.main, cs.side2, c->ev_fork));
  {  // SameNoiseLevels blur input + blur (sigma 10.67)
    SrcPack<SrcSameNoise, 1> s; PlanePack<1> t; CPlanePack<1> ct;
    s.s[0].a = p0.hf[1]; s.s[0].b = p1.hf[1];
    t.p[0] = c->tmp[0]; ct.p[0] = c->tmp[0];
    TRY((blur_h<23, SrcSameNoise, 1>(c, cs.side2, s, t, c->blur[B_SN])));
    PostStore<1> post; post.out[0] = c->snb;
    TRY((blur_v<23, 1, PostStore<1>>(c, cs.side2, ct, post, c->blur[B_SN])));
  }
  TRY(stage_mask_blurs(c, cs.side, cs.side2, mask_pack_psycho(c, p1)));
  TRY(record_for(c, cs.side, cs.main, c->ev_join));
  return record_for(c, cs.side2, cs.main, c->ev_join2);
}

// Who zeroes d_max_bits, which the chain's last kernel accumulates the image maximum into.
enum class ClearMax {
  kReconstruction,   // the full reconstruction at the head of this Compare has (its first workgroup)
  kCombine,          // k_combine does: a Compare on patched planes has no reconstruction in front
  kMemset,           // a fill in front of the last blur (a chain that starts behind the reconstruction: the probe)
};
// What a Compare is asked for (enqueue_compare; stage_diffmap reads the first two).
enum CompareWant : unsigned {
  kWantBlockMax = 1,   // the per-block maxima (d_block_max) beside the image maximum
  kWantDistmap = 2,    // the distance map stored in c->distmap
  kWholeChain = 4,     // never start from patched planes (gz_time_compare)
};

// DiffmapPsychoImage (butteraugli.cc:817-908) + score: p0 = original, p1 = candidate.
int stage_diffmap(gz_ctx* c, const ChainStreams& cs, const Psycho& p0, const Psycho& p1, unsigned want, ClearMax clear) {
  const float hf_asymmetry_ = 0.8f;
  // side streams: SameNoise blur + the mask branch; main stream: Malta
  TRY(fork_side_branch(c, cs, p0, p1));
  MaltaSpec ms[2][3];
  malta_specs(ms);
  dim3 mgrid(gz_div_up(c->w, MW), gz_div_up(c->h, MH), 2);
  MaltaArgs<3> ay, ax;
  for (int ch = 0; ch < 2; ++ch) {   // X, Y; passes in the reference's order: UHF, HF, MF
    MaltaArgs<3>& a = ch ? ay : ax;
    a.pass[0] = {p0.uhf[ch], p1.uhf[ch], ms[ch][0].nm, ms[ch][0].lf};
    a.pass[1] = {p0.hf[ch], p1.hf[ch], ms[ch][1].nm, ms[ch][1].lf};
    a.pass[2] = {p0.mf[ch], p1.mf[ch], ms[ch][2].nm, ms[ch][2].lf};
    a.out = c->ac[ch];
  }
  if (!c->batch.n) {
    GZ_LAUNCH((k_malta_rolled<3>), mgrid, dim3(256), cs.main, ay, ax, c->w, c->h, c->pitch);
  } else {
    mgrid.z *= c->batch.n;
    const BatchIdx bi = c->batch.idx;
    GZ_LAUNCH((k_malta_rolled_batch<3>), mgrid, dim3(256), cs.main, ay, ax, c->w, c->h, c->pitch, bi);
  }
  KCHK(c);
  TRY(wait_for(c, cs.side, cs.main, c->ev_join));
  TRY(wait_for(c, cs.side2, cs.main, c->ev_join2));
  {
    CombineArgs a = combine_mask_args(c, nullptr, nullptr);
    a.ac0 = c->ac[0]; a.ac1 = c->ac[1];
    a.lf0_x = p0.lfv[0]; a.lf1_x = p1.lfv[0];
    a.lf0_b = p0.lfv[2]; a.lf1_b = p1.lfv[2];
    const double wmul1 = 32.4449876135;
    a.sn_blur = c->snb;
    a.hf0_y = p0.hf[1];
    a.hf1_y = p1.hf[1];
    a.w_sn = 884.809801415;
    a.w_0gt1 = (wmul1 * hf_asymmetry_) * 0.8;   // L2DiffAsymmetric: w *= 0.8 (:678-679)
    a.w_0lt1 = (wmul1 / hf_asymmetry_) * 0.8;
    a.out = c->dsq;
    a.clear_word = clear == ClearMax::kCombine ? c->d_max_bits : nullptr;
    TRY(launch_combine(c, cs.main, a));
  }
  {  // CalculateDiffmap second half: blur(sigma 1.725, border_ratio 1.0) + mix
    SrcPack<SrcPlain, 1> s; s.s[0].p = c->dsq;
    PostDiffmapMix post; post.d = c->dsq; post.out = (want & kWantDistmap) ? c->distmap : nullptr;
    // (a batched chain: one image-maximum word per image, c->batch.max_bits, and no block maxima)
    unsigned* const max_bits = c->batch.n ? c->batch.max_bits : c->d_max_bits;
    if (clear == ClearMax::kMemset) HIPCHK(c, hipMemsetAsync(max_bits, 0, sizeof(unsigned) * (size_t)std::max(1, c->batch.n), cs.main));
    BlockMaxOut bm{(want & kWantBlockMax) ? c->d_block_max : nullptr, max_bits, c->bw, nullptr};
    TRY((blur2d<3, 1, SrcPlain, PostDiffmapMix, true>(c, cs.main, s, post, c->blur[B_FINAL], bm)));
  }
  return GZ_OK;
}

// k_scan_offsets' scratch for max_tiles tiles, as one allocation (zero before its first launch: ticket 0, no epoch yet).
inline size_t scan_state_bytes(int max_tiles) { return (size_t)max_tiles * (8 + 8 + 4) + 64; }
inline ScanState scan_state_at(void* d_state, int max_tiles) {
  ScanState st;
  st.agg = (unsigned long long*)d_state;
  st.incl = st.agg + max_tiles;
  st.status = (unsigned*)(st.incl + max_tiles);
  st.ticket = st.status + max_tiles;
  return st;
}
// The epoch of the scratch's next launch on `stream`, *epoch being the one of its last launch (0: none yet).  The
// flags keep 30 bits of it: where it would wrap, the scratch is cleared behind the launches before and the count starts
// over at 1.
inline hipError_t scan_next_epoch(unsigned* epoch, void* d_state, size_t bytes, hipStream_t stream) {
  if (++*epoch >= 0x3fffffffu) {
    const hipError_t e = hipMemsetAsync(d_state, 0, bytes, stream);
    if (e != hipSuccess) return e;
    *epoch = 1;
  }
  return hipSuccess;
}

// Exclusive 64-bit prefix sums of n 32-bit values on `stream` (which: 0 = the main stream's
// scratch, 1 = the entropy stream's).
int enqueue_scan_offsets(gz_ctx* c, int which, hipStream_t stream, const unsigned* d_bits, int n,
                         unsigned long long* d_off) {
  const int max_tiles = gz_div_up(c->nb, kScanTile) + 1;
  const size_t bytes = scan_state_bytes(max_tiles);
  if (!c->made.scan_state[which]) {
    TRY(regrow(c, stream, nullptr, 0, {{&c->d_scan_state[which], bytes}}));
    HIPCHK(c, hipMemsetAsync(c->d_scan_state[which], 0, bytes, stream));   // ticket 0, no epoch yet
    c->scan_epoch[which] = 0;
    c->made.scan_state[which] = true;
  }
  const ScanState st = scan_state_at(c->d_scan_state[which], max_tiles);
  HIPCHK(c, scan_next_epoch(&c->scan_epoch[which], c->d_scan_state[which], bytes, stream));
  const unsigned ep = c->scan_epoch[which];
  if (n > max_tiles * kScanTile) { c->err = "scan larger than its scratch"; return GZ_E_STATE; }
  GZ_LAUNCH(k_scan_offsets, dim3(std::max(1, gz_div_up(n, kScanTile))), dim3(256), stream, d_bits, n, d_off, st, ep);
  KCHK(c);
  return GZ_OK;
}

int stage_chroma_samples(gz_ctx* c, hipStream_t stream, const int16_t* d_coeffs) {
  if (!c->d_csamp) TRY(regrow(c, nullptr, nullptr, 0, {{(void**)&c->d_csamp, 2 * csamp_plane(c)}}));
  GZ_LAUNCH(k_chroma_samples, dim3(gz_div_up(c->nbc, kBlocksPerWG)), dim3(256), stream,
            d_coeffs + (size_t)c->coff[1] * 64, d_coeffs + (size_t)c->coff[2] * 64, c->cbw, c->nbc,
            c->d_csamp);
  KCHK(c);
  return GZ_OK;
}

int stage_reconstruct(gz_ctx* c, hipStream_t stream, const int16_t* d_coeffs, float* lin0, uint8_t* srgb,
                      unsigned* clear_word = nullptr) {
  if (c->cfac == 2) {
    TRY(stage_chroma_samples(c, stream, d_coeffs));
    GZ_LAUNCH(k_reconstruct420, dim3(c->bh * gz_div_up(c->bw, 8)), dim3(256), stream,
              d_coeffs, (const uint8_t*)c->d_csamp, c->w, c->h, c->bw, c->nb, c->cbw, c->cbh,
              c->pitch, c->plane, c->d_srgb_lut, lin0, srgb, clear_word);
    KCHK(c);
    return GZ_OK;
  }
  // strips of 8 blocks per workgroup: as many (up to 4) as leave the chip ~2000 workgroups (8 per CU)
  const int strips = gz_div_up(c->bw, kReconBlocks);
  int per = 4;
  while (per > 1 && (long)c->bh * gz_div_up(strips, per) < 2000) per >>= 1;
#ifdef GZ_EMU
  if (const char* e = getenv("GZ_EMU_RECON_STRIPS")) per = std::max(1, atoi(e));   // (the strip loop on images the emulation can afford)
#endif
  GZ_LAUNCH(k_reconstruct, dim3(c->bh * gz_div_up(strips, per)), dim3(256), stream,
            d_coeffs, c->w, c->h, c->bw, c->nb, c->pitch, c->plane, c->d_srgb_lut, lin0,
            srgb, clear_word, per);
  KCHK(c);
  return GZ_OK;
}

// ---------------------------------------------------------------- the self-checks -----
// (gz_config.patch_reconstruct == 2) What the calls between two Compares kept current is compared, word for word, with
// the same planes computed as a whole.  WordDiff: three scratch planes for the whole computation and the device's
// count of differing 32-bit words, from the pool for the length of a check.
static std::atomic<unsigned long long> g_compares{0}, g_compares_patched{0}, g_patch_checks{0};   // gz_compare_counters
static std::atomic<unsigned long long> g_compares_ahead{0}, g_ahead_checks{0};
struct WordDiff {
  float* planes = nullptr;
  unsigned* d_bad = nullptr;
  WordDiff() = default;
  WordDiff(const WordDiff&) = delete;
  WordDiff& operator=(const WordDiff&) = delete;
  ~WordDiff() { (void)pool_free(planes); (void)pool_free(d_bad); }
};
static int word_diff_begin(gz_ctx* c, hipStream_t stream, WordDiff* wd) {
  HIPCHK(c, pool_malloc((void**)&wd->planes, sizeof(float) * c->plane * 3));
  HIPCHK(c, pool_malloc((void**)&wd->d_bad, sizeof(unsigned)));
  HIPCHK(c, hipMemsetAsync(wd->d_bad, 0, sizeof(unsigned), stream));
  return GZ_OK;
}
static void word_diff_count(hipStream_t stream, const WordDiff& wd, const float* a, const float* b, size_t words) {
  unsigned* d_bad = wd.d_bad;
  GZ_LAUNCH(k_count_differing_words, dim3(1024), dim3(256), stream, (const unsigned*)a, (const unsigned*)b, words, d_bad);
}
static int word_diff_end(gz_ctx* c, hipStream_t stream, const WordDiff& wd, unsigned* bad) {
  HIPCHK(c, hipMemcpyAsync(bad, wd.d_bad, sizeof(unsigned), hipMemcpyDeviceToHost, stream));
  HIPCHK(c, hipStreamSynchronize(stream));
  return GZ_OK;
}
// lin[] as the patches left it against a full reconstruction of the candidate.
static int check_patched_planes(gz_ctx* c, hipStream_t stream) {
  WordDiff wd;
  unsigned bad = 0;
  TRY(word_diff_begin(c, stream, &wd));
  float* full = wd.planes;
  const int strips = gz_div_up(c->bw, kReconBlocks);
  GZ_LAUNCH(k_reconstruct, dim3(c->bh * strips), dim3(256), stream, (const int16_t*)c->d_cand, c->w, c->h, c->bw, c->nb,
            c->pitch, c->plane, (const float*)c->d_srgb_lut, full, (uint8_t*)nullptr, (unsigned*)nullptr, 1);
  word_diff_count(stream, wd, c->lin[0], full, (size_t)c->plane * 3);
  TRY(word_diff_end(c, stream, wd, &bad));
  ++g_patch_checks;
  if (bad) { c->err = "patched linear planes differ from a full reconstruction"; return GZ_E_STATE; }
  return GZ_OK;
}
// xyb[] as the calls kept it against the opsin blur of lin[] as a whole.
static int check_opsin_ahead(gz_ctx* c, hipStream_t stream) {
  WordDiff wd;
  unsigned bad = 0;
  TRY(word_diff_begin(c, stream, &wd));
  for (int i = 0; i < 3; ++i)
    HIPCHK(c, hipMemcpyAsync(wd.planes + (size_t)i * c->plane, c->xyb[i], sizeof(float) * c->plane, hipMemcpyDeviceToDevice, stream));
  TRY(stage_opsin(c, stream));
  for (int i = 0; i < 3; ++i) word_diff_count(stream, wd, c->xyb[i], wd.planes + (size_t)i * c->plane, (size_t)c->plane);
  TRY(word_diff_end(c, stream, wd, &bad));
  ++g_ahead_checks;
  if (bad) { c->err = "the opsin image kept ahead differs from the opsin blur of the whole planes"; return GZ_E_STATE; }
  return GZ_OK;
}

// One full Compare of the current candidate, everything on the stream (and, forked, the two side streams).
// want without kWantDistmap (the search loop, gz_time_compare): the last kernel leaves the per-block maxima and the
// image maximum only; c->distmap then holds no distance map (have_map_plane).
// The candidate's linear planes: reconstructed here, unless every change of the candidate since the last full
// reconstruction was patched into them by the call that made it (c->lin_is_cand; the search loop's steady state:
// a fifth of a 4K image's blocks change per iteration).  kWholeChain: gz_time_compare, whose repetitions change
// nothing and must not measure a chain without its first kernel.
int enqueue_compare(gz_ctx* c, unsigned want) {
  if (c->cfg.store_distmap != 0) want |= kWantDistmap;   // (1: the chain as it was until round 5, A/B)
  c->compare_forked = !single_stream_wanted(c);
  const ChainStreams cs = chain_streams(c, c->compare_forked);
  ++g_compares;
  const bool patched = !(want & kWholeChain) && c->cfg.patch_reconstruct != 0 && c->lin_is_cand && c->cfac == 1;
  if (patched) {
    if (c->cfg.patch_reconstruct == 2) TRY(check_patched_planes(c, cs.main));
    ++g_compares_patched;
  } else {
    TRY(stage_reconstruct(c, cs.main, c->d_cand, c->lin[0], nullptr, c->d_max_bits));
    c->lin_is_cand = c->cfac == 1 && c->cfg.patch_reconstruct != 0 && (c->nb >= 8192 || c->cfg.patch_reconstruct == 2);
  }
  // ... and their opsin image, when the same calls have kept that current too (xyb_is_cand; consumed here)
  const bool ahead = patched && c->xyb_is_cand;
  c->xyb_is_cand = false;
  if (ahead) {
    if (c->cfg.patch_reconstruct == 2) TRY(check_opsin_ahead(c, cs.main));
    ++g_compares_ahead;
  } else {
    TRY(stage_opsin(c, cs.main));
  }
  TRY(stage_separate(c, cs, &c->pi1));
  return stage_diffmap(c, cs, c->pi0, c->pi1, want, patched ? ClearMax::kCombine : ClearMax::kReconstruction);
}

int upload_planes(gz_ctx* c, const float* host, float* const* dev, int n) {
  for (int i = 0; i < n; ++i)
    HIPCHK(c, hipMemcpyAsync(dev[i], host + (size_t)i * c->w * c->h,
                             sizeof(float) * c->w * c->h, hipMemcpyHostToDevice, c->stream));
  return GZ_OK;
}
int download_plane(gz_ctx* c, const float* dev, float* host) {
  HIPCHK(c, hipMemcpyAsync(host, dev, sizeof(float) * c->w * c->h, hipMemcpyDeviceToHost,
                           c->stream));
  return GZ_OK;
}

int ensure_pip(gz_ctx* c) {
  if (c->have_pip) return GZ_OK;
  TRY(regrow(c, nullptr, nullptr, 0, {{(void**)&c->extra_arena, sizeof(float) * c->plane * 17}}));
  for (int i = 0; i < 17; ++i) c->free_planes.push_back(c->extra_arena + (size_t)i * c->plane);
  alloc_psycho(c, &c->pip);
  for (int i = 0; i < 3; ++i) { c->mask_out[i] = take_plane(c); c->mask_dc_out[i] = take_plane(c); }
  for (int i = 0; i < 2; ++i) c->sup_scratch[i] = take_plane(c);
  c->have_pip = true;
  return GZ_OK;
}


// StartBlockComparisons (butteraugli_comparator.cc:415-421): mask_xyz_ =
// Mask(opsin(orig), opsin(orig)).mask; only the values at block corners are ever read
// (CompareBlock, :484-486).
int ensure_block_mask(gz_ctx* c) {
  if (c->have_block_mask) return GZ_OK;
  TRY(byte_original(c, "StartBlockComparisons' mask"));   // (it is Mask() of d_rgb)
  TRY(ensure_pip(c));
  if (!c->d_block_mask) TRY(regrow(c, nullptr, nullptr, 0, {{(void**)&c->d_block_mask, sizeof(float) * 3 * c->nb}}));
  const hipStream_t stream = c->stream;
  dim3 grid(gz_div_up(c->w, 256), c->h);
  c->lin_is_cand = c->xyb_is_cand = false;   // (lin[] takes the original)
  GZ_LAUNCH(k_linear_from_rgb8, grid, dim3(256), stream, c->d_rgb, c->w, c->h, c->pitch,
            c->plane, c->d_srgb_lut, c->lin[0]);
  KCHK(c);
  TRY(stage_opsin(c, stream));
  MaskPrePack pk;
  {
    const float* const x2[2] = {c->xyb[0], c->xyb[1]};
    TRY(mask_pack_plain(c, stream, x2, x2, &pk));
  }
  TRY(stage_mask_blurs(c, stream, stream, pk));
  TRY(launch_combine(c, stream, combine_mask_args(c, c->mask_out, nullptr)));
  GZ_LAUNCH(k_gather_block_corners, dim3(gz_div_up(c->nb, 256)), dim3(256), stream,
            (const float*)c->mask_out[0], (const float*)c->mask_out[1],
            (const float*)c->mask_out[2], c->pitch, c->bw, c->nb, c->d_block_mask);
  KCHK(c);
  c->have_block_mask = true;
  return GZ_OK;
}

}  // namespace
