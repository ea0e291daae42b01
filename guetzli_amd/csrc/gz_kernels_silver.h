// Params::use_silver_screen on the device: RGBToYUV420 (guetzli/preprocess_downsample.cc:452-476),
// the YUV 4:2:0 samples whose decoded image has the original's luma when averaged in linear light,
// found by twenty rounds through the decoder model.  host/silver_screen.cc is the same conversion
// plane by plane on the host; here one thread owns a 2 x 2 cell -- one chroma sample and its (up to)
// four luma samples -- and runs a round's stages for it in registers, every expression with the
// reference's operand types and order (gz_silver_ref.h holds them once for both sides).
//
// Every float the reference computes is static_cast<float>(pow(...)) of glibc's pow.  The device's pow
// is another function, so each evaluation goes through gz_pow_to_float_guarded (gz_math.h), which
// proves that both round to the same float or says that it cannot.  A cell with one unproven power
// writes nothing and appends itself to a list; k_silver_gather then packs what the host needs to
// redo it with libm, and k_silver_patch scatters the host's results before the next round starts
// (api/entry_frame.h: silver_run).  About 5e-4 of the cell-rounds take that way.
#pragma once
#include "gz_math.h"
#include "gz_silver_ref.h"

namespace gz {

constexpr int kSilverRounds = 20;
constexpr int kSilverChunk = 1024;   // cells per gather / patch pass through the pinned staging
constexpr int kSilverIn = 26;        // floats of a gathered cell: rec[4][3], guess_y[4], y_target[4], gu, gv, tu, tv, nx, ny
constexpr int kSilverOut = 8;        // floats the host returns per cell (k_silver_patch)
constexpr int kSilverHeader = 16;    // floats in front of the staging's records: [0] the list's length

struct SilverArgs {
  int w, h, w2, h2;         // image, chroma grid = cells
  const uint8_t* rgb;       // packed sRGB, the input
  const float* lut;         // GammaToLinear of a byte (built by the host's libm)
  float* y_target;          // [h][w]
  float* guess_y;           // [h][w], updated in place
  float* target_u;          // [h2][w2]
  float* target_v;
  float* guess_u[2];        // ping-pong: a round reads one half (its neighbours' old values) and writes the other
  float* guess_v[2];
  unsigned* list;           // [0]: number of listed cells, [1 + i]: their indices (capacity: every cell)
  double guard;             // G of gz_pow_to_float_guarded
  int list_all;             // every cell takes the host path (the test of gather / patch)
};

// The two powers of a cell on the device.  kInit: the samples are bytes and GammaToLinear comes from the table.
template <bool kInit>
struct SilverDevPow {
  const float* lut;
  double guard;
  bool ambiguous;
  GZ_DEVFN float to_linear(float x) {
    if (kInit) return lut[(int)x];
    bool a;
    const float r = gz_pow_to_float_guarded((double)(x / 255.0f), gz_silver::kGammaExp, 1.0, guard, &a, nullptr);
    ambiguous |= a;
    return r;
  }
  GZ_DEVFN float to_gamma(float x) {
    bool a;
    const float r = gz_pow_to_float_guarded((double)x, gz_silver::kInvGammaExp, 255.0, guard, &a, nullptr);
    ambiguous |= a;
    return r;
  }
};

struct SilverCellPos { int cx, cy, nx, ny; };
GZ_DEVFN SilverCellPos silver_cell_pos(const SilverArgs& a, int cell) {
  SilverCellPos p;
  p.cy = cell / a.w2;
  p.cx = cell - p.cy * a.w2;
  p.nx = 2 * p.cx + 1 < a.w ? 2 : 1;
  p.ny = 2 * p.cy + 1 < a.h ? 2 : 1;
  return p;
}

// The cell's pixels as floats of the input bytes (slots outside the image: zero, never read).
GZ_DEVFN void silver_rec_from_bytes(const SilverArgs& a, const SilverCellPos& p, float rec[4][3]) {
  for (int s = 0; s < 4; ++s) {
    const int iy = s >> 1, ix = s & 1;
    const bool in = iy < p.ny && ix < p.nx;
    const size_t i = in ? 3 * ((size_t)(2 * p.cy + iy) * a.w + (2 * p.cx + ix)) : 0;
    for (int c = 0; c < 3; ++c) rec[s][c] = in ? (float)a.rgb[i + c] : 0.0f;
  }
}
// ... and as YUV420ToRGB (:428-437) decodes the current guess: BoxUpsample + Blur ("fancy upsample") of the chroma
// guess read at half resolution -- the box-upsampled plane at (y0, clamp(x0 +- 2)) IS the neighbouring cell's sample,
// clamped to the grid -- then the colour matrix and Clip.
GZ_DEVFN void silver_rec_from_guess(const SilverArgs& a, const SilverCellPos& p, int from, float rec[4][3]) {
  const float* gu = a.guess_u[from];
  const float* gv = a.guess_v[from];
  const int xl = p.cx > 0 ? p.cx - 1 : 0, xr = p.cx + 1 < a.w2 ? p.cx + 1 : a.w2 - 1;
  const int yt = p.cy > 0 ? p.cy - 1 : 0, yb = p.cy + 1 < a.h2 ? p.cy + 1 : a.h2 - 1;
  const size_t row = (size_t)p.cy * a.w2;
  const float u0 = gu[row + p.cx], v0 = gv[row + p.cx];
  for (int s = 0; s < 4; ++s) {
    const int iy = s >> 1, ix = s & 1;
    if (iy < p.ny && ix < p.nx) {
      const int xn = ix ? xr : xl;
      const size_t rown = (size_t)(iy ? yb : yt) * a.w2;
      const float u = gz_silver::Fancy(u0, gu[row + xn], gu[rown + p.cx], gu[rown + xn]);
      const float v = gz_silver::Fancy(v0, gv[row + xn], gv[rown + p.cx], gv[rown + xn]);
      gz_silver::YuvToRgb(a.guess_y[(size_t)(2 * p.cy + iy) * a.w + (2 * p.cx + ix)], u, v, rec[s]);
    } else {
      rec[s][0] = rec[s][1] = rec[s][2] = 0.0f;
    }
  }
}

GZ_DEVFN void silver_list_cell(const SilverArgs& a, int cell) {
  const unsigned at = atomicAdd(a.list, 1u);   // (at most one entry per cell and launch: the capacity is every cell)
  a.list[1 + at] = (unsigned)cell;
}

// y_target, the downsampled target, the first guesses (:454-458).
__global__ __launch_bounds__(256) void k_silver_init(SilverArgs a) {
  const int cell = blockIdx.x * 256 + threadIdx.x;
  if (cell >= a.w2 * a.h2) return;
  const SilverCellPos p = silver_cell_pos(a, cell);
  float rec[4][3], yrec[4], yuv[3];
  silver_rec_from_bytes(a, p, rec);
  SilverDevPow<true> pw = {a.lut, a.guard, false};
  gz_silver::CellEval(rec, p.nx, p.ny, pw, yrec, yuv);
  if (pw.ambiguous || a.list_all) { silver_list_cell(a, cell); return; }
  for (int s = 0; s < 4; ++s) {
    const int iy = s >> 1, ix = s & 1;
    if (iy < p.ny && ix < p.nx) {
      const size_t i = (size_t)(2 * p.cy + iy) * a.w + (2 * p.cx + ix);
      a.y_target[i] = yrec[s];
      a.guess_y[i] = yuv[0];   // (BoxUpsample of the target's luma)
    }
  }
  a.target_u[cell] = a.guess_u[0][cell] = yuv[1];
  a.target_v[cell] = a.guess_v[0][cell] = yuv[2];
}

// One round (:459-471): decode the guess, take its luma and its downsampled pixel, move the guess by the difference
// to the targets.  Reads half `from` of the chroma guess, writes the other one.
__global__ __launch_bounds__(256) void k_silver_iter(SilverArgs a, int from) {
  const int cell = blockIdx.x * 256 + threadIdx.x;
  if (cell >= a.w2 * a.h2) return;
  const SilverCellPos p = silver_cell_pos(a, cell);
  float rec[4][3], yrec[4], yuv[3];
  silver_rec_from_guess(a, p, from, rec);
  SilverDevPow<false> pw = {a.lut, a.guard, false};
  gz_silver::CellEval(rec, p.nx, p.ny, pw, yrec, yuv);
  if (pw.ambiguous || a.list_all) { silver_list_cell(a, cell); return; }
  for (int s = 0; s < 4; ++s) {
    const int iy = s >> 1, ix = s & 1;
    if (iy < p.ny && ix < p.nx) {
      const size_t i = (size_t)(2 * p.cy + iy) * a.w + (2 * p.cx + ix);
      a.guess_y[i] = gz_silver::Update(a.guess_y[i], yrec[s], a.y_target[i]);
    }
  }
  a.guess_u[from ^ 1][cell] = gz_silver::Update(a.guess_u[from][cell], yuv[1], a.target_u[cell]);
  a.guess_v[from ^ 1][cell] = gz_silver::Update(a.guess_v[from][cell], yuv[2], a.target_v[cell]);
}

// Listed cells [first, first + kSilverChunk) of the list, as far as it goes: what the host needs to redo each
// (the listed cells wrote nothing, so guess_y and half `from` are still the round's input).  from < 0: the init
// pass, whose input is the bytes.  stage: pinned and mapped; [0] receives the list's length.
__global__ __launch_bounds__(256) void k_silver_gather(SilverArgs a, int from, unsigned first, float* stage) {
  const unsigned n = a.list[0];
  const unsigned t = blockIdx.x * 256 + threadIdx.x;
  if (t == 0) reinterpret_cast<unsigned*>(stage)[0] = n;
  if (t >= (unsigned)kSilverChunk || first + t >= n) return;
  const int cell = (int)a.list[1 + first + t];
  const SilverCellPos p = silver_cell_pos(a, cell);
  float rec[4][3];
  if (from < 0) silver_rec_from_bytes(a, p, rec); else silver_rec_from_guess(a, p, from, rec);
  float* o = stage + kSilverHeader + (size_t)t * kSilverIn;
  for (int s = 0; s < 4; ++s) {
    const int iy = s >> 1, ix = s & 1;
    const bool in = iy < p.ny && ix < p.nx && from >= 0;
    const size_t i = in ? (size_t)(2 * p.cy + iy) * a.w + (2 * p.cx + ix) : 0;
    for (int c = 0; c < 3; ++c) o[3 * s + c] = rec[s][c];
    o[12 + s] = in ? a.guess_y[i] : 0.0f;
    o[16 + s] = in ? a.y_target[i] : 0.0f;
  }
  o[20] = from >= 0 ? a.guess_u[from][cell] : 0.0f;
  o[21] = from >= 0 ? a.guess_v[from][cell] : 0.0f;
  o[22] = from >= 0 ? a.target_u[cell] : 0.0f;
  o[23] = from >= 0 ? a.target_v[cell] : 0.0f;
  o[24] = (float)p.nx;
  o[25] = (float)p.ny;
}

// The host's results for the n listed cells from `first` on, kSilverOut floats each (res: pinned and mapped).
// Init pass (from < 0): y_target[4], yuv[3]; a round: the new guess_y[4], guess_u, guess_v.
__global__ __launch_bounds__(256) void k_silver_patch(SilverArgs a, int from, unsigned first, unsigned n, const float* res) {
  const unsigned t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const int cell = (int)a.list[1 + first + t];
  const SilverCellPos p = silver_cell_pos(a, cell);
  const float* r = res + (size_t)t * kSilverOut;
  for (int s = 0; s < 4; ++s) {
    const int iy = s >> 1, ix = s & 1;
    if (iy < p.ny && ix < p.nx) {
      const size_t i = (size_t)(2 * p.cy + iy) * a.w + (2 * p.cx + ix);
      if (from < 0) { a.y_target[i] = r[s]; a.guess_y[i] = r[4]; } else { a.guess_y[i] = r[s]; }
    }
  }
  if (from < 0) {
    a.target_u[cell] = a.guess_u[0][cell] = r[5];
    a.target_v[cell] = a.guess_v[0][cell] = r[6];
  } else {
    a.guess_u[from ^ 1][cell] = r[4];
    a.guess_v[from ^ 1][cell] = r[5];
  }
}

// Upsample2x2 (:384-402) of the final chroma guesses into full planes.
__global__ __launch_bounds__(256) void k_silver_upsample(const float* gu, const float* gv, int w, int h, int w2,
                                                        float* out_u, float* out_v) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= w || y >= h) return;
  const size_t s = (size_t)(y >> 1) * w2 + (x >> 1), o = (size_t)y * w + x;
  out_u[o] = gu[s];
  out_v[o] = gv[s];
}

// gz_pow_to_float_guarded element-wise (gz_probe_math, GZ_MATH_POW_TO_FLOAT): out[0][i] = the device's p,
// out[1][i] = the float as a double, out[2][i] = 1.0 where it is ambiguous.
__global__ __launch_bounds__(256) void k_probe_pow(const double* base, int n, double expo, double scale, double guard,
                                                  double* out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  bool amb;
  double p;
  const float f = gz_pow_to_float_guarded(base[i], expo, scale, guard, &amb, &p);
  out[i] = p;
  out[(size_t)n + i] = (double)f;
  out[2 * (size_t)n + i] = amb ? 1.0 : 0.0;
}

}  // namespace gz
