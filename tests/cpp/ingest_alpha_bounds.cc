// TEST ONLY (CPU, host sanitizers): gz_pack_rgb_device_pixels -- the ingest kernels k_ingest_rgba and k_ingest_rgb<uint16>
// of gz_kernels_ingest.h through their launch code -- over every layout, element type and width the tests use, on colour
// and alpha sources malloc'ed to EXACTLY their last addressed element + 1.  Built with -DGZ_EMU
// -fsanitize=address,undefined against tests/emu/hip_emu.h: a read of a 16-byte path or of a row's tail that leaves
// [0, (h-1) sy + (w-1) sx + 2 sc] of the colours or [0, (h-1) sy + (w-1) sx] of alpha is a heap-buffer-overflow report, a
// misaligned 16-byte access an alignment report.  The bytes are checked against the rule restated here as well:
// byte = the value (uint8), v >> 8 (uint16), rint(clamp(x * 255, 0, 255)) (floats); out = (v a + bg (255 - a) + 128) / 255.
//
// A stand-alone program: nothing is loaded into another process, no preloaded runtime.
#include "../../guetzli_amd/csrc/gz_api.hip"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// (the emulation keeps its fibers' stacks for the life of the process: not what this program looks for)
extern "C" const char* __asan_default_options() { return "detect_leaks=0"; }

namespace {

struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 32);
  }
};

size_t elem_size(int dtype) { return dtype == GZ_DT_U8 ? 1 : dtype == GZ_DT_F32 ? 4 : 2; }

// a finite float16: (1024 + m) * 2^(e - 25), or m * 2^-24 for a subnormal -- exact in float
float widen_f16(uint16_t h) {
  const int e = (h >> 10) & 31, m = h & 0x3ff;
  const float mag = std::ldexp((float)(e ? 1024 + m : m), (e ? e : 1) - 25);
  return (h & 0x8000) ? -mag : mag;
}

// the expected byte of the sample whose storage is `bits`
uint8_t expected_byte(int dtype, uint32_t bits) {
  if (dtype == GZ_DT_U8) return (uint8_t)bits;
  if (dtype == GZ_DT_U16) return (uint8_t)(bits >> 8);
  float x;
  if (dtype == GZ_DT_F32) {
    memcpy(&x, &bits, 4);
  } else if (dtype == GZ_DT_BF16) {
    const uint32_t u = bits << 16;
    memcpy(&x, &u, 4);
  } else {
    const uint16_t h = (uint16_t)bits;
    if (((h >> 10) & 31) == 31) {
      const uint32_t u = ((uint32_t)(h & 0x8000) << 16) | 0x7f800000u | ((uint32_t)(h & 0x3ff) << 13);
      memcpy(&x, &u, 4);
    } else {
      x = widen_f16(h);
    }
  }
  volatile float v = x * 255.0f;
  if (std::isnan(v)) return 0;
  if (v < 0.0f) return 0;
  if (v > 255.0f) return 255;
  return (uint8_t)std::nearbyint((float)v);
}

uint8_t expected_blend(int v, int a, int bg) { return (uint8_t)((v * a + bg * (255 - a) + 128) / 255); }

// storage bits of a random sample: floats mostly in [0, 1], some bit patterns of every kind
uint32_t random_bits(int dtype, Rng* r) {
  const uint32_t u = r->next();
  if (dtype == GZ_DT_U8) return u & 0xff;
  if (dtype == GZ_DT_U16) return u & 0xffff;
  if ((u & 7) == 0) return dtype == GZ_DT_F32 ? r->next() : r->next() & 0xffff;
  const float x = (float)(r->next() & 0xffff) / 65535.0f;
  uint32_t f;
  memcpy(&f, &x, 4);
  if (dtype == GZ_DT_F32) return f;
  if (dtype == GZ_DT_BF16) return f >> 16;
  // f32 in [0, 1] -> f16 by truncation (any f16 will do)
  const int e = (int)((f >> 23) & 0xff) - 127 + 15;
  if (e <= 0) return 0;
  return ((uint32_t)e << 10) | ((f >> 13) & 0x3ff);
}

// `count` random samples in an allocation of exactly that many
void* random_source(int dtype, size_t count, Rng* rng) {
  const size_t elem = elem_size(dtype);
  void* mem = malloc(count * elem);   // (16-byte aligned: the offsets alone decide which read path the launch code may take)
  if (!mem) return nullptr;
  for (size_t i = 0; i < count; ++i) {
    const uint32_t b = random_bits(dtype, rng);
    if (elem == 1) ((uint8_t*)mem)[i] = (uint8_t)b;
    else if (elem == 2) ((uint16_t*)mem)[i] = (uint16_t)b;
    else ((uint32_t*)mem)[i] = b;
  }
  return mem;
}

uint32_t bits_at(const void* mem, size_t elem, size_t i) {
  return elem == 1 ? ((const uint8_t*)mem)[i] : elem == 2 ? ((const uint16_t*)mem)[i] : ((const uint32_t*)mem)[i];
}

// where the pixels sit: `n` channels interleaved (HWC) or planar (CHW), whole or a crop of a canvas, base + 0 or + 1
enum Kind { kHwcRgba, kChwRgba, kGreyAlphaInterleaved, kChwGreyAlpha, kAlphaApart, kOpaque };
struct Layout { const char* name; Kind kind; bool crop; int base1; int opaque_kind; };
const Layout kAlphaLayouts[] = {
    {"HWC RGBA", kHwcRgba, false, 0, 0},          {"HWC RGBA crop", kHwcRgba, true, 0, 0},          {"HWC RGBA base+1", kHwcRgba, false, 1, 0},
    {"CHW RGBA", kChwRgba, false, 0, 0},          {"CHW RGBA crop", kChwRgba, true, 0, 0},          {"CHW RGBA base+1", kChwRgba, false, 1, 0},
    {"grey+alpha", kGreyAlphaInterleaved, false, 0, 0}, {"grey+alpha crop", kGreyAlphaInterleaved, true, 0, 0}, {"grey+alpha base+1", kGreyAlphaInterleaved, false, 1, 0},
    {"CHW grey+alpha", kChwGreyAlpha, false, 0, 0}, {"CHW grey+alpha crop", kChwGreyAlpha, true, 0, 0}, {"CHW grey+alpha base+1", kChwGreyAlpha, false, 1, 0},
    {"alpha apart", kAlphaApart, false, 0, 0},    {"alpha apart crop", kAlphaApart, true, 0, 0},    {"alpha apart base+1", kAlphaApart, false, 1, 0}};
// the opaque layouts of ingest_bounds.cc: 0 HWC, 1 CHW, 2 HWC crop, 3 CHW crop, 4 grey, 5 HWC + 1, 6 CHW crop + 1
const Layout kOpaqueLayouts[] = {{"opaque HWC", kOpaque, false, 0, 0}, {"opaque CHW", kOpaque, false, 0, 1}, {"opaque HWC crop", kOpaque, true, 0, 2},
                                 {"opaque CHW crop", kOpaque, true, 0, 3}, {"opaque grey", kOpaque, false, 0, 4}, {"opaque HWC base+1", kOpaque, false, 1, 5},
                                 {"opaque CHW crop base+1", kOpaque, true, 1, 6}};

int run_case(int dtype, const Layout& lay, int w, int h, Rng* rng, long* cases) {
  const size_t elem = elem_size(dtype);
  const int64_t W = lay.crop ? (w + 16 + 15) / 16 * 16 : w, H = lay.crop ? h + 2 : h;   // the canvas: rows of a multiple of 16 pixels
  const int64_t first = lay.crop ? 1 * W + 16 : 0;                                      // the canvas pixel that is (0, 0)
  int64_t sy, sx, sc, lead, alead = -1;   // lead / alead: elements of the allocation in front of (0, 0, 0) / of alpha's (0, 0)
  bool apart = false;
  switch (lay.kind) {
    case kHwcRgba: sy = 4 * W; sx = 4; sc = 1; lead = 4 * first; alead = lead + 3; break;
    case kChwRgba: sy = W; sx = 1; sc = W * H; lead = first; alead = lead + 3 * W * H; break;
    case kGreyAlphaInterleaved: sy = 2 * W; sx = 2; sc = 0; lead = 2 * first; alead = lead + 1; break;
    case kChwGreyAlpha: sy = W; sx = 1; sc = 0; lead = first; alead = lead + W * H; break;
    case kAlphaApart: sy = W; sx = 1; sc = W * H; lead = first; alead = first; apart = true; break;
    default:
      switch (lay.opaque_kind) {
        case 0: case 2: case 5: sy = 3 * W; sx = 3; sc = 1; lead = 3 * first; break;
        case 1: case 3: case 6: sy = W; sx = 1; sc = W * H; lead = first; break;
        default: sy = W; sx = 1; sc = 0; lead = first; break;
      }
      break;
  }
  lead += lay.base1;
  if (alead >= 0) alead += lay.base1;
  const int64_t plane = (int64_t)(h - 1) * sy + (int64_t)(w - 1) * sx;
  // one allocation ends at the later of the last colour element and (alpha inside it) the last alpha element
  int64_t count = lead + plane + 2 * sc + 1;
  if (alead >= 0 && !apart && alead + plane + 1 > count) count = alead + plane + 1;
  void* mem = random_source(dtype, (size_t)count, rng);
  void* amem = apart ? random_source(dtype, (size_t)(alead + plane + 1), rng) : mem;
  if (!mem || !amem) return 2;
  gz_device_pixels img;
  memset(&img, 0, sizeof(img));
  img.struct_size = (int)sizeof(img);
  img.dtype = dtype;
  img.data = (const char*)mem + (size_t)lead * elem;
  img.stride_y = sy; img.stride_x = sx; img.stride_c = sc;
  img.alpha = alead >= 0 ? (const char*)amem + (size_t)alead * elem : nullptr;
  for (int c = 0; c < 3; ++c) img.background[c] = (uint8_t)rng->next();
  std::vector<uint8_t> out((size_t)3 * w * h, 0xEE);
  const int rc = gz_pack_rgb_device_pixels(0, &img, w, h, out.data());
  int bad = rc != GZ_OK;
  for (int y = 0; y < h && !bad; ++y)
    for (int x = 0; x < w && !bad; ++x)
      for (int c = 0; c < 3; ++c) {
        const uint32_t b = bits_at(mem, elem, (size_t)(lead + y * sy + x * sx + c * sc));
        uint8_t exp = expected_byte(dtype, b);
        if (alead >= 0) exp = expected_blend(exp, expected_byte(dtype, bits_at(amem, elem, (size_t)(alead + y * sy + x * sx))), img.background[c]);
        if (out[((size_t)y * w + x) * 3 + c] != exp) {
          printf("MISMATCH dtype %d %s %dx%d at (%d, %d, %d): bits %08x -> %d, expected %d\n", dtype, lay.name, w, h, y, x, c, b,
                 out[((size_t)y * w + x) * 3 + c], exp);
          bad = 1;
          break;
        }
      }
  if (apart) free(amem);
  free(mem);
  ++*cases;
  return bad;
}

}  // namespace

int main() {
  const int widths[] = {1, 3, 4, 5, 15, 16, 17, 33, 61, 64, 67}, heights[] = {1, 2, 9};
  Rng rng{20261019};
  long cases = 0;
  int bad = 0;
  for (int dtype = GZ_DT_U8; dtype <= GZ_DT_U16; ++dtype)
    for (const Layout& lay : kAlphaLayouts)
      for (int w : widths)
        for (int h : heights) bad |= run_case(dtype, lay, w, h, &rng, &cases);
  for (const Layout& lay : kOpaqueLayouts)   // uint16 without alpha: k_ingest_rgb's new instantiation
    for (int w : widths)
      for (int h : heights) bad |= run_case(GZ_DT_U16, lay, w, h, &rng, &cases);
  printf("%ld cases, %s\n", cases, bad ? "FAILED" : "all bytes as expected, no read outside the sources");
  return bad;
}
