// TEST ONLY (CPU, host sanitizers): the distance map's emit kernel k_emit_map of gz_kernels_emitmap.h through its launch
// code, over every layout, element type and size the tests use, from source planes malloc'ed to EXACTLY w * h floats
// (and one float further on, so that no row starts 16-byte aligned) into destinations malloc'ed to EXACTLY the last
// addressed element + 1.  Built with -DGZ_EMU -fsanitize=address,undefined against tests/emu/hip_emu.h: a 16-byte load
// or store, or a row's tail, that leaves its buffer is a heap-buffer-overflow report, a misaligned 16-byte access an
// alignment report.  The elements are checked against the rounding restated here in floating point, and the elements of
// a canvas that are no part of the image against the sentinel they were filled with.
//
// A stand-alone program: nothing is loaded into another process, no preloaded runtime.
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

// float -> float16 bits by scaling and nearbyint (round to nearest even is the default mode); NaN: 0xffff
uint32_t ref_f16(float f) {
  if (std::isnan(f)) return 0xffffu;
  const uint32_t sign = std::signbit(f) ? 0x8000u : 0u;
  const double a = std::fabs((double)f);
  if (a >= 65520.0) return sign | 0x7c00u;
  if (a < std::ldexp(1.0, -14)) return sign | (uint32_t)std::nearbyint(std::ldexp(a, 24));   // subnormals, 0, and 0x400 by the carry
  int e = 0;
  const double m = std::frexp(a, &e);                      // a = m 2^e, m in [0.5, 1)
  uint32_t mant = (uint32_t)std::nearbyint(std::ldexp(m, 11));   // 1024 .. 2048
  if (mant == 2048u) { mant = 1024u; ++e; }
  return sign | ((uint32_t)(e + 14) << 10) | (mant - 1024u);
}
// float -> bfloat16 bits: the float whose low 16 bits are zero that is nearest, ties to the even upper half
uint32_t ref_bf16(float f) {
  if (std::isnan(f)) return 0xffffu;
  uint32_t u;
  memcpy(&u, &f, 4);
  const uint32_t low = u & 0xffffu;
  uint32_t hi = u >> 16;
  if (low > 0x8000u || (low == 0x8000u && (hi & 1u))) ++hi;
  return hi;
}
uint32_t expected_bits(int dtype, float f) {
  if (dtype == kF16) return ref_f16(f);
  if (dtype == kBF16) return ref_bf16(f);
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}
bool is_nan_bits(int dtype, uint32_t b) {
  if (dtype == kF16) return (b & 0x7fffu) > 0x7c00u;
  if (dtype == kBF16) return (b & 0x7fffu) > 0x7f80u;
  return (b & 0x7fffffffu) > 0x7f800000u;
}

struct Layout { const char* name; int kind; };   // 0 contiguous, 1 crop, 2 base + 1, 3 pitch + 1, 4 transposed
const Layout kLayouts[] = {{"contiguous", 0}, {"crop", 1}, {"base+1", 2}, {"pitch+1", 3}, {"transposed", 4}};

uint32_t load(const void* mem, size_t elem, size_t i) { return elem == 2 ? ((const uint16_t*)mem)[i] : ((const uint32_t*)mem)[i]; }

int run_case(int dtype, const Layout& lay, int w, int h, int src_lead, long* cases) {
  const size_t elem = dtype == kF32 ? 4 : 2;
  const int64_t cw = (w + 16 + 15) / 16 * 16;   // the canvas of a crop: rows of a multiple of 16 elements
  int64_t sy = w, sx = 1, lead = 0;             // lead: elements in front of (0, 0) that belong to the allocation
  switch (lay.kind) {
    case 1: sy = cw; lead = cw + 16; break;
    case 2: lead = 1; break;
    case 3: sy = w + 1; break;
    case 4: sy = 1; sx = h; break;
    default: break;
  }
  const int64_t last = (int64_t)(h - 1) * sy + (int64_t)(w - 1) * sx;
  const size_t count = (size_t)(lead + last + 1);
  // malloc returns 16-byte aligned memory, so `lead` and `src_lead` alone decide which paths the kernel may take
  void* mem = malloc(count * elem);
  float* plane = (float*)malloc(sizeof(float) * ((size_t)w * h + src_lead));
  if (!mem || !plane) return 2;
  memset(mem, 0xEE, count * elem);
  float* src = plane + src_lead;
  uint64_t s = 88172645463325252ull + (uint64_t)w * 131 + (uint64_t)h;
  const float special[] = {0.0f, 1e-6f, 5.9604645e-8f, 2.9802322e-8f, 6.1035156e-5f, 65504.0f, 65519.0f, 65520.0f, 1e30f, INFINITY, -INFINITY, NAN,
                           -1.5f, 3.3895314e38f, 1.0f, 0.33333334f};
  for (size_t i = 0; i < (size_t)w * h; ++i) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    src[i] = (s >> 60) == 0 ? special[(s >> 40) % 16] : (float)((s >> 33) % 100000) * 3e-4f;
  }
  std::vector<uint8_t> is_image(count, 0);
  int bad = 0;
  void* out = (char*)mem + (size_t)lead * elem;
  if (dtype == kF32) gz::launch_emit_map((hipStream_t) nullptr, src, w, h, w, (float*)out, sy, sx);
  else if (dtype == kF16) gz::launch_emit_map((hipStream_t) nullptr, src, w, h, w, (gz::ingest_f16*)out, sy, sx);
  else gz::launch_emit_map((hipStream_t) nullptr, src, w, h, w, (gz::ingest_bf16*)out, sy, sx);
  for (int y = 0; y < h && !bad; ++y)
    for (int x = 0; x < w; ++x) {
      const size_t i = (size_t)(lead + y * sy + x * sx);
      is_image[i] = 1;
      const float f = src[(size_t)y * w + x];
      const uint32_t got = load(mem, elem, i), exp = expected_bits(dtype, f);
      if (std::isnan(f) ? !is_nan_bits(dtype, got) : got != exp) {
        printf("MISMATCH dtype %d %s %dx%d at (%d, %d): %a -> %08x, expected %08x\n", dtype, lay.name, w, h, y, x, (double)f, got, exp);
        bad = 1;
        break;
      }
    }
  const uint32_t sentinel = elem == 2 ? 0xEEEEu : 0xEEEEEEEEu;
  for (size_t i = 0; i < count && !bad; ++i)
    if (!is_image[i] && load(mem, elem, i) != sentinel) {
      printf("TOUCHED dtype %d %s %dx%d: element %zu outside the image is %08x\n", dtype, lay.name, w, h, i, load(mem, elem, i));
      bad = 1;
    }
  free(mem);
  free(plane);
  ++*cases;
  return bad;
}

}  // namespace

int main() {
  const int widths[] = {8, 9, 15, 16, 17, 33, 61, 64, 67}, heights[] = {8, 9, 17};
  long cases = 0;
  int bad = 0;
  for (int dtype = kF32; dtype <= kBF16; ++dtype)
    for (const Layout& lay : kLayouts)
      for (int w : widths)
        for (int h : heights)
          for (int src_lead = 0; src_lead < 2; ++src_lead) bad |= run_case(dtype, lay, w, h, src_lead, &cases);
  printf("%ld cases, %s\n", cases, bad ? "FAILED" : "all elements as expected, no access outside the buffers");
  return bad;
}
