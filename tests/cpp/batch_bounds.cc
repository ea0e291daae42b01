// TEST ONLY (CPU, host sanitizers): the batched forms of the Compare chain's kernels (gz_common.h, BatchIdx / BatchTensor)
// through the emulation's launch -- the batched ingest, one batched k_blur2d (the opsin blur), a batched row / column
// pair (radius 16), the batched k_combine with ONE reference for all images (ref_stride 0) and the batched emit -- on
// N = 3 images of 9 x 17 and 67 x 33.  The source tensor, the arenas, the reference's planes and the destination are
// malloc'ed to EXACTLY their last element: the arenas end with the last image's last plane, not with a whole stride.
// Built with -DGZ_EMU -fsanitize=address,undefined against tests/emu/hip_emu.h: an access of image i that leaves the
// buffers is a heap-buffer-overflow report, a misaligned 16-byte access an alignment report.  What the batched launches
// leave in every plane of every arena, and in the destination, is compared bit for bit with the same kernels launched
// once per image on arenas of their own; the floats between two arenas keep their sentinel.
//
// A stand-alone program: nothing is loaded into another process, no preloaded runtime.
#include "../../guetzli_amd/csrc/gz_kernels_ingest.h"
#include "../../guetzli_amd/csrc/gz_kernels_blur.h"
#include "../../guetzli_amd/csrc/gz_kernels_diff.h"
#include "../../guetzli_amd/csrc/gz_kernels_emitmap.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// (the emulation keeps its fibers' stacks for the life of the process: not what this program looks for)
extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }

using namespace gz;

namespace {

constexpr int kPlanes = 9;   // lin[3], xyb[3], the row pass's result, the column pass's, k_combine's
constexpr int kN = 3;
const hipStream_t kStream = (hipStream_t) nullptr;

template <int R>
Taps<R> some_taps() {
  Taps<R> t;
  float sum = 0.0f;
  for (int j = 0; j <= 2 * R; ++j) { t.k[j] = 1.0f / (1.0f + (float)((j - R) * (j - R))); sum += t.k[j]; }
  for (int j = 0; j <= 2 * R; ++j) t.ks[j] = t.k[j] * (1.0f / sum);
  return t;
}
// border scales of exactly R floats each
struct Scales {
  std::vector<float*> owned;
  BorderScale make(int r) {
    BorderScale b;
    float* lo = (float*)malloc(sizeof(float) * r);
    float* hi = (float*)malloc(sizeof(float) * r);
    for (int i = 0; i < r; ++i) { lo[i] = 1.0f + 0.01f * i; hi[i] = 1.0f + 0.02f * i; }
    owned.push_back(lo); owned.push_back(hi);
    b.lo = lo; b.hi = hi;
    return b;
  }
  ~Scales() { for (float* p : owned) free(p); }
};

struct Tables {
  float lut[256];
  std::vector<double> mask;
  Tables() : mask(2048) {
    for (int i = 0; i < 256; ++i) lut[i] = (float)i * 1.0039f;
    for (int i = 0; i < 2048; ++i) mask[i] = 0.5 + 0.001 * (i % 512);
  }
};

// The five launches on `n` images whose arenas start `stride` floats apart at `arena`, batched (one launch each) or --
// n == 1, batched == false -- as the kernels of one image.
void run_chain(bool batched, int n, const uint8_t* src, float* arena, size_t stride, const float* ref3, float* dst, int w, int h, const Tables& tb,
               Scales* sc) {
  const int pitch = w;
  const size_t plane = (size_t)pitch * h;
  float* P[kPlanes];
  for (int i = 0; i < kPlanes; ++i) P[i] = arena + (size_t)i * plane;
  const BatchIdx bi = {stride, 0};
  const long long sy = 3 * w, sx = 3, sc_ = 1, sn = (long long)3 * w * h;
  {  // ingest: uint8 NHWC, element by element and by 16-byte vectors where the layout allows
    const int wide = sn % 16 == 0 ? ingest_wide_mode(src, 1, sy, sx, sc_) : (int)kIngestElementwise;
    const dim3 grid((unsigned)(((size_t)gz_div_up(w, 16) * h + 255) / 256), (unsigned)n), block(256);
    const float* lut = tb.lut;
    float* lin = P[0];
    if (batched) {
      const BatchTensor bt = {sn, stride};
      uint8_t* const none = nullptr;
      GZ_LAUNCH((k_ingest_rgb<uint8_t, BatchTensor>), grid, block, kStream, src, sy, sx, sc_, w, h, wide, none, lut, lin, pitch, plane, bt);
    } else {
      std::vector<uint8_t> bytes((size_t)3 * w * h);
      uint8_t* rgb = bytes.data();
      GZ_LAUNCH((k_ingest_rgb<uint8_t>), grid, block, kStream, src, sy, sx, sc_, w, h, wide, rgb, lut, lin, pitch, plane);
    }
  }
  {  // the opsin blur: k_blur2d<2, 3>
    SrcPack<SrcPlain, 3> s;
    PostOpsin post;
    for (int i = 0; i < 3; ++i) { s.s[i].p = P[i]; post.lin[i] = P[i]; post.xyb[i] = P[3 + i]; }
    const Taps<2> tp = some_taps<2>();
    const BorderScale bx = sc->make(2), by = sc->make(2);
    const BlockMaxOut bm{nullptr, nullptr, 0, nullptr};
    const dim3 grid(gz_div_up(w, T2), gz_div_up(h, 16), batched ? n : 1);
    if (batched) GZ_LAUNCH((k_blur2d<2, 3, SrcPlain, PostOpsin, false, 16, BatchIdx>), grid, dim3(256), kStream, s, post, w, h, pitch, tp, bx, by, bm, bi);
    else GZ_LAUNCH((k_blur2d<2, 3, SrcPlain, PostOpsin, false, 16>), grid, dim3(256), kStream, s, post, w, h, pitch, tp, bx, by, bm);
  }
  {  // a row pass and a column pass of radius 16
    SrcPack<SrcPlain, 1> s; PlanePack<1> t; CPlanePack<1> ct; PostStore<1> post;
    s.s[0].p = P[4]; t.p[0] = P[6]; ct.p[0] = P[6]; post.out[0] = P[7];
    const Taps<16> tp = some_taps<16>();
    const BorderScale bx = sc->make(16), by = sc->make(16);
    const dim3 hgrid(gz_div_up(w, HW), gz_div_up(h, HH), batched ? n : 1), vgrid(gz_div_up(w, VW), gz_div_up(h, 16), batched ? n : 1);
    if (batched) {
      GZ_LAUNCH((k_blur_h<16, SrcPlain, 1, false, BatchIdx>), hgrid, dim3(256), kStream, s, t, w, h, pitch, tp, bx, tp, bx, bi);
      GZ_LAUNCH((k_blur_v_compact<16, 1, PostStore<1>, 16, false, BatchIdx>), vgrid, dim3(256), kStream, ct, post, w, h, pitch, tp, by, tp, by, bi);
    } else {
      GZ_LAUNCH((k_blur_h<16, SrcPlain, 1, false>), hgrid, dim3(256), kStream, s, t, w, h, pitch, tp, bx, tp, bx);
      GZ_LAUNCH((k_blur_v_compact<16, 1, PostStore<1>, 16, false>), vgrid, dim3(256), kStream, ct, post, w, h, pitch, tp, by, tp, by);
    }
  }
  {  // k_combine: the reference's three planes are ONE image's for all (ref_stride 0)
    CombineArgs a;
    memset(&a, 0, sizeof(a));
    a.mask_x_blur = P[0]; a.mask_y_blur1 = P[1]; a.mask_y_blur2 = P[2];
    a.ac0 = P[0]; a.ac1 = P[1];
    a.lf0_x = ref3; a.lf1_x = P[3];
    a.lf0_b = ref3 + plane; a.lf1_b = P[5];
    a.sn_blur = P[7]; a.hf0_y = ref3 + 2 * plane; a.hf1_y = P[4];
    a.w_sn = 2.0; a.w_0gt1 = 3.0; a.w_0lt1 = 5.0;
    a.luts = tb.mask.data();
    a.out = P[8];
    const dim3 grid(gz_div_up(w, 1024), h, batched ? n : 1);
    if (batched) GZ_LAUNCH((k_combine<BatchIdx>), grid, dim3(256), kStream, a, w, h, pitch, bi);
    else GZ_LAUNCH(k_combine, grid, dim3(256), kStream, a, w, h, pitch);
  }
  {  // the emit: float32 maps, contiguous [n][h][w]
    const long long msn = (long long)w * h, msy = w, msx = 1;
    const bool wide = msn % 4 == 0 && emit_map_wide(dst, 4, msy, msx);
    const dim3 grid((unsigned)(((size_t)((w + 3) / 4) * h + 255) / 256), (unsigned)n), block(256);
    const float* map = P[8];
    if (batched) {
      const BatchTensor bt = {msn, stride};
      if (wide) GZ_LAUNCH((k_emit_map<float, true, BatchTensor>), grid, block, kStream, map, w, h, pitch, dst, msy, msx, bt);
      else GZ_LAUNCH((k_emit_map<float, false, BatchTensor>), grid, block, kStream, map, w, h, pitch, dst, msy, msx, bt);
    } else {
      if (wide) GZ_LAUNCH((k_emit_map<float, true>), grid, block, kStream, map, w, h, pitch, dst, msy, msx);
      else GZ_LAUNCH((k_emit_map<float, false>), grid, block, kStream, map, w, h, pitch, dst, msy, msx);
    }
  }
}

int run_case(int w, int h, size_t gap, long* cases) {
  const size_t plane = (size_t)w * h;
  // the arenas' stride: the planes rounded up to 4 floats, plus `gap` further multiples of 4 that belong to nobody
  const size_t stride = ((plane * kPlanes + 3) & ~(size_t)3) + 4 * gap;
  const size_t arena_floats = stride * (kN - 1) + plane * kPlanes;   // EXACTLY up to the last image's last element
  uint8_t* src = (uint8_t*)malloc((size_t)kN * 3 * plane);
  float* arena = (float*)malloc(sizeof(float) * arena_floats);
  float* ref3 = (float*)malloc(sizeof(float) * 3 * plane);
  float* dst = (float*)malloc(sizeof(float) * kN * plane);
  if (!src || !arena || !ref3 || !dst) return 2;
  uint64_t s = 88172645463325252ull + (uint64_t)w * 131 + (uint64_t)h;
  for (size_t i = 0; i < (size_t)kN * 3 * plane; ++i) { s = s * 6364136223846793005ull + 1442695040888963407ull; src[i] = (uint8_t)(s >> 56); }
  for (size_t i = 0; i < 3 * plane; ++i) { s = s * 6364136223846793005ull + 1442695040888963407ull; ref3[i] = (float)((s >> 40) % 1000) * 0.01f; }
  const float sentinel = -12345.5f;
  for (size_t i = 0; i < arena_floats; ++i) arena[i] = sentinel;
  const Tables tb;
  Scales sc;
  int bad = 0;
  run_chain(true, kN, src, arena, stride, ref3, dst, w, h, tb, &sc);
  for (int i = 0; i < kN && !bad; ++i) {
    float* own = (float*)malloc(sizeof(float) * plane * kPlanes);
    float* own_dst = (float*)malloc(sizeof(float) * plane);
    // (a copy of image i at an address as aligned as the batch's: the same read path)
    uint8_t* own_src = (uint8_t*)malloc(3 * plane + 16);
    uint8_t* at = own_src + ((uintptr_t)(src + (size_t)i * 3 * plane) & 15u);
    memcpy(at, src + (size_t)i * 3 * plane, 3 * plane);
    run_chain(false, 1, at, own, 0, ref3, own_dst, w, h, tb, &sc);
    for (int p = 0; p < kPlanes && !bad; ++p)
      if (memcmp(own + (size_t)p * plane, arena + (size_t)i * stride + (size_t)p * plane, sizeof(float) * plane) != 0) {
        printf("MISMATCH %dx%d gap %zu: image %d, plane %d differs from the kernel of one image\n", w, h, gap, i, p);
        bad = 1;
      }
    if (!bad && memcmp(own_dst, dst + (size_t)i * plane, sizeof(float) * plane) != 0) {
      printf("MISMATCH %dx%d gap %zu: map %d differs from the kernel of one image\n", w, h, gap, i);
      bad = 1;
    }
    for (size_t k = plane * kPlanes; i + 1 < kN && k < stride && !bad; ++k)
      if (memcmp(&arena[(size_t)i * stride + k], &sentinel, sizeof(float)) != 0) {
        printf("TOUCHED %dx%d gap %zu: float %zu between arenas %d and %d\n", w, h, gap, k, i, i + 1);
        bad = 1;
      }
    free(own); free(own_dst); free(own_src);
  }
  free(src); free(arena); free(ref3); free(dst);
  ++*cases;
  return bad;
}

}  // namespace

int main() {
  const int shapes[][2] = {{9, 17}, {67, 33}, {64, 32}};   // (64 x 32: pitch and plane multiples of 4 -- the 16-byte paths)
  long cases = 0;
  int bad = 0;
  for (const auto& sh : shapes)
    for (size_t gap = 0; gap < 2; ++gap) bad |= run_case(sh[0], sh[1], gap, &cases);
  printf("%ld cases, %s\n", cases, bad ? "FAILED" : "all elements as expected, no access outside the buffers");
  return bad;
}
