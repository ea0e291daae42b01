// The per-sample functions of RGBToYUV420 (guetzli/preprocess_downsample.cc:283-319), every
// expression with the reference's operand types and association.  ONE copy for the three places
// that evaluate them: host/silver_screen.cc (the whole conversion on the host), the kernels of
// gz_kernels_silver.h (Clip and the colour matrices; their powers go through gz_pow_to_float), and
// the host code of gz_api.hip that redoes the cells whose device power could not be proven to
// round like libm's (the libm forms below).  Plain C++: no HIP type, no library but libm.
#pragma once
#include <math.h>

#if defined(__HIPCC__) && !defined(GZ_EMU)
#define GZ_SILVER_FN __host__ __device__ inline
#else
#define GZ_SILVER_FN inline
#endif

namespace gz_silver {

// std::max(0.0f, std::min(255.0f, v)), spelled out (std::min / std::max return their FIRST argument unless
// the second compares smaller / larger)
GZ_SILVER_FN float Clip(float v) {
  const float m = v < 255.0f ? v : 255.0f;
  return 0.0f < m ? m : 0.0f;
}
GZ_SILVER_FN float ToY(float r, float g, float b) { return 0.299f * r + 0.587f * g + 0.114f * b; }
GZ_SILVER_FN float ToU(float r, float g, float b) { return -0.16874f * r - 0.33126f * g + 0.5f * b + 128.0f; }
GZ_SILVER_FN float ToV(float r, float g, float b) { return 0.5f * r - 0.41869f * g - 0.08131f * b + 128.0f; }
// YUV420ToRGB's pixel (:428-437) from its luma and the fancy-upsampled chroma
GZ_SILVER_FN void YuvToRgb(float y, float u, float v, float* rgb) {
  rgb[0] = Clip(y + 1.402f * (v - 128.0f));
  rgb[1] = Clip(y - 0.344136f * (u - 128.0f) - 0.714136f * (v - 128.0f));
  rgb[2] = Clip(y + 1.772f * (u - 128.0f));
}
// Blur's tap sum (:405-426): the cell's own sample a, its horizontal, vertical and diagonal neighbours
GZ_SILVER_FN float Fancy(float a, float b, float c, float d) {
  return (9.0f * a + 3.0f * b + 3.0f * c + 1.0f * d) / 16.0f;
}
// UpdateGuess (:439-448)
GZ_SILVER_FN float Update(float guess, float rec, float target) { return Clip(guess - (rec - target)); }

// The argument and the scale of the two powers: GammaToLinear(x) = float(1.0 * pow(x / 255.0f, 2.2)),
// LinearToGamma(x) = float(255.0 * pow(x, 1.0 / 2.2)).
constexpr double kGammaExp = 2.2;
constexpr double kInvGammaExp = 1.0 / 2.2;

// libm's own: host code only
inline float GammaToLinear(float x) { return static_cast<float>(pow(x / 255.0f, 2.2)); }
inline float LinearToGamma(float x) { return static_cast<float>(255.0 * pow(x, 1.0 / 2.2)); }
struct LibmPow {
  float to_linear(float x) { return GammaToLinear(x); }
  float to_gamma(float x) { return LinearToGamma(x); }
};

// One 2 x 2 cell of LinearlyAveragedLuma (:321-330) and RGBToYUV(LinearlyDownsample2x2(rgb)) (:332-367) from its
// pixels rec[slot][channel], slot = 2 * iy + ix: yrec[slot] the luma of every pixel, yuv[3] the downsampled pixel.
// nx, ny (1 or 2): the cell's columns and rows inside the image; a slot outside is the edge pixel again, as the
// downsample's min(h - 1, 2y + iy) / min(w - 1, 2x + ix) reads it (rec of such a slot is not read).  The twelve
// GammaToLinear values serve both results: the same function of the same inputs.  P supplies the two powers
// (LibmPow above; the kernels' guarded device power).  Constant indices only: everything stays in registers.
template <class P>
GZ_SILVER_FN void CellEval(const float (*rec)[3], int nx, int ny, P& pw, float* yrec, float* yuv) {
  float lin[4][3];
#define GZ_SILVER_EVAL(p)                                                  \
  do {                                                                     \
    lin[p][0] = pw.to_linear(rec[p][0]);                                   \
    lin[p][1] = pw.to_linear(rec[p][1]);                                   \
    lin[p][2] = pw.to_linear(rec[p][2]);                                   \
    yrec[p] = pw.to_gamma(ToY(lin[p][0], lin[p][1], lin[p][2]));           \
  } while (0)
#define GZ_SILVER_COPY(p, s)                                               \
  do {                                                                     \
    lin[p][0] = lin[s][0]; lin[p][1] = lin[s][1]; lin[p][2] = lin[s][2];   \
    yrec[p] = yrec[s];                                                     \
  } while (0)
  GZ_SILVER_EVAL(0);
  if (nx > 1) GZ_SILVER_EVAL(1); else GZ_SILVER_COPY(1, 0);
  if (ny > 1) GZ_SILVER_EVAL(2); else GZ_SILVER_COPY(2, 0);
  if (nx > 1 && ny > 1) GZ_SILVER_EVAL(3);
  else if (ny > 1) GZ_SILVER_COPY(3, 2);
  else if (nx > 1) GZ_SILVER_COPY(3, 1);
  else GZ_SILVER_COPY(3, 0);
#undef GZ_SILVER_EVAL
#undef GZ_SILVER_COPY
  float px[3];
  for (int c = 0; c < 3; ++c) {
    float acc = 0.0f;
    acc += lin[0][c];
    acc += lin[1][c];
    acc += lin[2][c];
    acc += lin[3][c];
    px[c] = pw.to_gamma(0.25f * acc);
  }
  yuv[0] = ToY(px[0], px[1], px[2]);
  yuv[1] = ToU(px[0], px[1], px[2]);
  yuv[2] = ToV(px[0], px[1], px[2]);
}

}  // namespace gz_silver
