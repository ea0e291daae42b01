// gz_pow_to_float (guetzli_amd/csrc/gz_math.h) against libm, on the host: the guard's claim is that a result it
// does not call ambiguous is static_cast<float>(scale * pow(base, expo)) of libm -- whatever the device's own pow
// returned, as long as that is within G = 2^-40 of the true power.  The emulation's pow IS libm's, so the device's
// is played by libm's moved by gz_emu_pow_ulps() = -1000, 0, +1000 double ulps (2^-42 relative at the most: inside G,
// and 60 times what OpenCL allows a double pow).  Swept over every stride-th float argument of the two uses:
//   GammaToLinear(x) = float(1.0 * pow(x / 255.0f, 2.2)),        x in [0, 255]   (denormal arguments included)
//   LinearToGamma(x) = float(255.0 * pow(x, 1.0 / 2.2)),         x in [0, 1 + 2^-20]
// Stand-alone: g++ -DGZ_EMU -Iguetzli_amd/csrc -Itests/emu (optionally -fsanitize=address,undefined).
// usage: silver_guard [stride]   (default 997)
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gz_math.h"

static float from_bits(unsigned u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}
static unsigned to_bits(float f) {
  unsigned u;
  memcpy(&u, &f, 4);
  return u;
}

struct Tally { unsigned long long n = 0, ambiguous = 0, wrong = 0; };

// mode 0: GammaToLinear, 1: LinearToGamma
static void sweep(int mode, unsigned stride, int skew, Tally* t, bool guarded = true) {
  gz::gz_emu_pow_ulps() = skew;
  const unsigned last = to_bits(mode == 0 ? 255.0f : 1.0f + 0x1p-20f);
  for (unsigned long long b = 0; b <= last; b += stride) {
    const float x = from_bits((unsigned)b);
    const double base = mode == 0 ? (double)(x / 255.0f) : (double)x;
    const double expo = mode == 0 ? 2.2 : 1.0 / 2.2, scale = mode == 0 ? 1.0 : 255.0;
    bool amb = false;
    const float got = guarded ? gz::gz_pow_to_float(base, expo, scale, &amb)
                              : gz::gz_pow_to_float_guarded(base, expo, scale, 0.0, &amb, nullptr);
    const float want = static_cast<float>(scale * pow(base, expo));
    ++t->n;
    if (amb) { ++t->ambiguous; continue; }
    if (to_bits(got) != to_bits(want)) {
      if (t->wrong++ < 5 && guarded) printf("  mode %d skew %d x %a: got %a want %a\n", mode, skew, x, got, want);
    }
  }
  gz::gz_emu_pow_ulps() = 0;
}

int main(int argc, char** argv) {
  const unsigned stride = argc > 1 ? (unsigned)strtoul(argv[1], nullptr, 10) : 997u;
  if (stride == 0) return 2;
  int bad = 0;
  for (int mode = 0; mode < 2; ++mode)
    for (int skew : {-1000, 0, 1000}) {
      Tally t;
      sweep(mode, stride, skew, &t);
      printf("%s skew %+5d: %llu arguments, %llu ambiguous (%.2e), %llu mismatches\n",
             mode == 0 ? "GammaToLinear" : "LinearToGamma", skew, t.n, t.ambiguous, (double)t.ambiguous / (double)t.n, t.wrong);
      // the guard must not pass everything to the host either: 2.4e-5 is expected for uniform arguments, and the
      // sweep's are log-uniform (the float grid), where tiny results that round to 0 or to a denormal add none
      if (t.wrong != 0 || t.ambiguous * 1000 > t.n) bad = 1;
    }
  // the control: without the guard the same skew does change floats (about 1000 * 2^-29 of them: a dozen at four
  // times the density), so the sweeps above would have seen a guard that proves nothing
  {
    Tally t;
    for (int mode = 0; mode < 2; ++mode)
      for (int skew : {-1000, 1000}) sweep(mode, stride / 4 + 1, skew, &t, false);
    printf("control, guard off: %llu arguments, %llu mismatches\n", t.n, t.wrong);
    if (t.wrong == 0 || t.ambiguous != 0) bad = 1;
  }
  // exact results are never ambiguous, whatever the skew
  gz::gz_emu_pow_ulps() = 1000;
  for (double expo : {2.2, 1.0 / 2.2})
    for (double base : {0.0, 1.0}) {
      bool amb = true;
      const float got = gz::gz_pow_to_float(base, expo, 255.0, &amb);
      if (amb || got != (float)(255.0 * base)) { printf("exact case pow(%g, %g) failed\n", base, expo); bad = 1; }
    }
  gz::gz_emu_pow_ulps() = 0;
  printf(bad ? "FAILED\n" : "every unambiguous result is libm's\n");
  return bad;
}
