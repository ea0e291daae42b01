// TEST ONLY (CPU, host sanitizers): the linear ingest kernel k_ingest_linear of gz_kernels_ingestlin.h through its launch
// code -- every layout, element type and width the tests use, and the extension of images under 8 pixels -- from
// sources malloc'ed to EXACTLY the last addressed element + 1 into planes malloc'ed to EXACTLY 3 * w * h floats; and
// k_region_max of gz_kernels_emitmap.h over windows of a plane malloc'ed to its last float.  Built with -DGZ_EMU
// -fsanitize=address,undefined against tests/emu/hip_emu.h: a 16-byte load or store, or a row's tail, that leaves its
// buffer is a heap-buffer-overflow report, a misaligned 16-byte access an alignment report.  The planes are checked
// against the value rule restated here, the count against the restatement's, the maximum against a loop.
//
// A stand-alone program: nothing is loaded into another process, no preloaded runtime.
#include "../../guetzli_amd/csrc/gz_kernels_ingestlin.h"
#include "../../guetzli_amd/csrc/gz_kernels_emitmap.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// (the emulation keeps its fibers' stacks for the life of the process: not what this program looks for)
extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }

namespace {

enum { kF32 = 0, kF16 = 1, kBF16 = 2 };

uint32_t bits_of(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}
float float_of(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}
// the exact widening of a storage element, by the formats' definitions (not the kernel's integer operations)
float widen(int dtype, uint32_t e) {
  if (dtype == kF32) return float_of(e);
  if (dtype == kBF16) return float_of(e << 16);
  const int sign = (e >> 15) & 1, ex = (e >> 10) & 31, m = e & 0x3ff;
  double v;
  if (ex == 31) v = m ? NAN : INFINITY;
  else if (ex == 0) v = std::ldexp((double)m, -24);
  else v = std::ldexp((double)(m + 1024), ex - 25);
  return (float)(sign ? -v : v);
}
// the value rule, and whether it altered the element
float rule(float x, float scale, unsigned* altered) {
  const volatile float v = x * scale;   // (one float32 multiplication)
  if (std::isnan(v) || v < 0.0f) { ++*altered; return 0.0f; }
  if (v > 255.0f) { ++*altered; return 255.0f; }
  return v;
}

struct Layout { const char* name; int kind; };   // 0 HWC, 1 CHW, 2 HWC crop at an odd element, 3 CHW crop at an odd element, 4 grey, 5 CHW crop (aligned)
const Layout kLayouts[] = {{"HWC", 0}, {"CHW", 1}, {"HWC crop + 1", 2}, {"CHW crop + 1", 3}, {"grey", 4}, {"CHW crop", 5}};

uint32_t element(uint64_t* s, int dtype) {
  static const float special[] = {NAN, -1.0f, -0.0f, 255.5f, INFINITY, -INFINITY, 0.0f, 255.0f, 1e-40f, 3e38f, -3e38f, 128.0f};
  *s = *s * 6364136223846793005ull + 1442695040888963407ull;
  const float f = (*s >> 60) == 0 ? special[(*s >> 40) % 12] : (float)((*s >> 33) % 25600) * 0.01f;
  if (dtype == kF32) return bits_of(f);
  if (dtype == kBF16) return bits_of(f) >> 16;
  // float16: any finite or special pattern will do -- every one of them has an exact widening
  return (*s >> 60) == 0 ? (uint32_t)((*s >> 20) & 0xffff) : (uint32_t)(0x3000 + ((*s >> 33) % 0x2b00));
}

void launch(int dtype, const void* data, long long sy, long long sx, long long sc, int w, int h, float scale, const gz::IngestExtent* ext,
            float* lin, unsigned* altered) {
  const hipStream_t st = (hipStream_t) nullptr;
  if (dtype == kF32) gz::launch_ingest_linear(st, (const float*)data, sy, sx, sc, w, h, scale, ext, lin, w, (size_t)w * h, altered);
  else if (dtype == kF16) gz::launch_ingest_linear(st, (const gz::ingest_f16*)data, sy, sx, sc, w, h, scale, ext, lin, w, (size_t)w * h, altered);
  else gz::launch_ingest_linear(st, (const gz::ingest_bf16*)data, sy, sx, sc, w, h, scale, ext, lin, w, (size_t)w * h, altered);
}

uint32_t load(const void* mem, size_t elem, size_t i) { return elem == 2 ? ((const uint16_t*)mem)[i] : ((const uint32_t*)mem)[i]; }
void store(void* mem, size_t elem, size_t i, uint32_t v) {
  if (elem == 2) ((uint16_t*)mem)[i] = (uint16_t)v;
  else ((uint32_t*)mem)[i] = v;
}

// One image of sw x sh source pixels in `lay`, ingested into a w x h canvas (extend: the rule for small images; else
// w x h is the image itself).
int run_case(int dtype, const Layout& lay, int sw, int sh, bool extend, float scale, long* cases) {
  const size_t elem = dtype == kF32 ? 4 : 2;
  const int64_t cw = (sw + 16 + 15) / 16 * 16, ch = sh + 2;
  int64_t sy = 0, sx = 0, sc = 0, lead = 0;
  switch (lay.kind) {
    case 0: sy = 3 * sw; sx = 3; sc = 1; break;
    case 1: sy = sw; sx = 1; sc = (int64_t)sw * sh; break;
    case 2: sy = 3 * cw; sx = 3; sc = 1; lead = (cw + 16) * 3 + 1; break;
    case 3: sy = cw; sx = 1; sc = ch * cw; lead = cw + 16 + 1; break;
    case 4: sy = sw; sx = 1; sc = 0; break;
    default: sy = cw; sx = 1; sc = ch * cw; lead = cw + 16; break;
  }
  const int64_t last = (int64_t)(sh - 1) * sy + (int64_t)(sw - 1) * sx + 2 * sc;
  const size_t count = (size_t)(lead + last + 1);
  const int w = extend && sw < 8 ? 8 : sw, h = extend && sh < 8 ? 8 : sh;
  const gz::IngestExtent ext = {sw, sh, sw < 8 ? (8 - sw) / 2 : 0, sh < 8 ? (8 - sh) / 2 : 0};
  // malloc returns 16-byte aligned memory, so `lead` alone decides which read path the kernel may take
  void* mem = malloc(count * elem);
  float* lin = (float*)malloc(sizeof(float) * 3 * (size_t)w * h);
  unsigned* altered = (unsigned*)malloc(sizeof(unsigned));
  if (!mem || !lin || !altered) return 2;
  uint64_t s = 88172645463325252ull + (uint64_t)sw * 131 + (uint64_t)sh + (uint64_t)dtype * 7;
  for (size_t i = 0; i < count; ++i) store(mem, elem, i, element(&s, dtype));
  for (size_t i = 0; i < 3 * (size_t)w * h; ++i) lin[i] = -12345.0f;
  *altered = 0;
  const void* data = (const char*)mem + (size_t)lead * elem;
  launch(dtype, data, sy, sx, sc, w, h, scale, extend ? &ext : nullptr, lin, altered);
  int bad = 0;
  unsigned expect_altered = 0;
  for (int c = 0; c < 3 && !bad; ++c)
    for (int y = 0; y < h && !bad; ++y)
      for (int x = 0; x < w; ++x) {
        int ys = y, xs = x;
        bool own = true;
        if (extend) {
          ys = y - ext.yborder; xs = x - ext.xborder;
          const int yc = ys < 0 ? 0 : (ys >= sh ? sh - 1 : ys), xc = xs < 0 ? 0 : (xs >= sw ? sw - 1 : xs);
          own = ys == yc && xs == xc;
          ys = yc; xs = xc;
        }
        unsigned one = 0;
        const float exp = rule(widen(dtype, load(mem, elem, (size_t)(lead + ys * sy + xs * sx + c * sc))), scale, &one);
        if (own) expect_altered += one;
        const float got = lin[((size_t)c * h + y) * w + x];
        if (bits_of(got) != bits_of(exp)) {
          printf("MISMATCH dtype %d %s %dx%d%s at (%d, %d, %d): %a, expected %a\n", dtype, lay.name, sw, sh, extend ? " extended" : "", y, x, c,
                 (double)got, (double)exp);
          bad = 1;
          break;
        }
      }
  if (!bad && *altered != expect_altered) {
    printf("COUNT dtype %d %s %dx%d%s: %u, expected %u\n", dtype, lay.name, sw, sh, extend ? " extended" : "", *altered, expect_altered);
    bad = 1;
  }
  free(mem);
  free(lin);
  free(altered);
  ++*cases;
  return bad;
}

// k_region_max over the window (x0, y0, w, h) of a plane of pitch floats per row that ends with the window's last float.
int run_region(int pitch, int x0, int y0, int w, int h, long* cases) {
  const size_t count = (size_t)(y0 + h - 1) * pitch + x0 + w;
  float* plane = (float*)malloc(sizeof(float) * count);
  unsigned* out = (unsigned*)malloc(sizeof(unsigned));
  if (!plane || !out) return 2;
  uint64_t s = 1234567ull + (uint64_t)w * 977 + (uint64_t)h;
  for (size_t i = 0; i < count; ++i) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    plane[i] = (float)((s >> 33) % 100000) * 3e-4f;
  }
  // the largest values of the plane lie OUTSIDE the window, right around it
  if (x0 > 0) plane[(size_t)y0 * pitch + x0 - 1] = 1e6f;
  if (y0 > 0) plane[(size_t)(y0 - 1) * pitch + x0] = 1e6f;
  if (x0 + w < pitch && h > 1) plane[(size_t)y0 * pitch + x0 + w] = 1e6f;
  float exp = 0.0f;
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) exp = std::fmax(exp, plane[(size_t)(y0 + y) * pitch + x0 + x]);
  *out = 0;
  gz::launch_region_max((hipStream_t) nullptr, plane, pitch, x0, y0, w, h, out);
  int bad = 0;
  if (*out != bits_of(exp)) {
    printf("REGION MAX pitch %d (%d, %d) %dx%d: %08x, expected %08x\n", pitch, x0, y0, w, h, *out, bits_of(exp));
    bad = 1;
  }
  free(plane);
  free(out);
  ++*cases;
  return bad;
}

}  // namespace

int main() {
  const int widths[] = {8, 9, 11, 15, 16, 17, 33, 64, 67}, heights[] = {8, 9};
  const int small[][2] = {{1, 1}, {3, 5}, {7, 9}, {9, 7}, {4, 40}, {7, 7}, {2, 8}};
  long cases = 0;
  int bad = 0;
  for (int dtype = kF32; dtype <= kBF16; ++dtype)
    for (const Layout& lay : kLayouts) {
      for (int w : widths)
        for (int h : heights) bad |= run_case(dtype, lay, w, h, false, (w & 1) ? 1.0f : 255.0f, &cases);
      for (const auto& sz : small) {
        bad |= run_case(dtype, lay, sz[0], sz[1], true, 1.0f, &cases);
        bad |= run_case(dtype, lay, sz[0], sz[1], false, 1.0f, &cases);   // (the kernel itself takes any size)
      }
    }
  for (const auto& sz : small) {
    const int w = sz[0], h = sz[1], cw = w < 8 ? 8 : w, xb = w < 8 ? (8 - w) / 2 : 0, yb = h < 8 ? (8 - h) / 2 : 0;
    bad |= run_region(cw, xb, yb, w, h, &cases);
  }
  bad |= run_region(300, 5, 3, 290, 7, &cases);   // several blocks, a partial last wavefront
  bad |= run_region(64, 0, 0, 64, 4, &cases);     // exactly one block
  printf("%ld cases, %s\n", cases, bad ? "FAILED" : "all elements as expected, no access outside the buffers");
  return bad;
}
