// Phase B's two-phase calls (tests/test_phase_b_protocol.py has the table) as plain C calls, for a run of the C ABI's
// host side under AddressSanitizer and UBSan with no interpreter in the process: the fused iteration as the search
// loop drives it, a begin that supersedes a begin, a new frame between begin and end, one failed launch, and two calls
// that run out of memory in the middle of a group made on first use and are repeated on the same context.
// Built by hand with the emulation of the kernels (tests/emu/hip_emu.h), not part of the suite (two minutes of g++):
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -DGZ_EMU
//       -Itests/emu -Iinclude -Wall -Wno-unused-function -Wno-unknown-pragmas -Wno-unused-variable
//       tests/cpp/phase_b_protocol_sanitized.cc -x c++ guetzli_amd/csrc/gz_api.hip -o phase_b_protocol_sanitized
// Exit status 0 and "ok" = every call returned what the table says; the sanitizers abort on their own findings.
// (The emulation keeps its fibers' stacks for the life of the process: LSAN_OPTIONS=suppressions=<a file that says
// leak:hipemu::launch>.)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "guetzli_amd.h"

extern "C" void gz_emu_fail_launch(long n);
extern "C" void gz_emu_fail_alloc(long n);

#define EXPECT(call, want)                                                                            \
  do {                                                                                                \
    const int rc_ = (call);                                                                           \
    if (rc_ != (want)) {                                                                              \
      fprintf(stderr, "%s:%d: %s = %d, expected %d (%s)\n", __FILE__, __LINE__, #call, rc_, (want),   \
              c ? gz_last_error(c) : "");                                                             \
      exit(1);                                                                                        \
    }                                                                                                 \
  } while (0)

static const int W = 100, H = 84, NB = 13 * 11, LEVELS = 12;
static const float TARGET = 0.971769f, PER_BLOCK = 2.0f;

// A context as phase B finds it: a candidate, phase A's block search, max_block_error zeroed, a distance map.
static gz_ctx* searched(uint64_t* candidates, bool reset = true) {
  std::vector<uint8_t> rgb((size_t)3 * W * H);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x)
      for (int ch = 0; ch < 3; ++ch)
        rgb[((size_t)y * W + x) * 3 + ch] = (uint8_t)(40 + ((x * (3 + ch) + y * (5 - ch)) % 97) + ((x / 8 + y / 8 + ch) % 2) * 90);
  int err = 0;
  gz_ctx* c = gz_create(0, W, H, rgb.data(), TARGET, &err);
  if (!c) { fprintf(stderr, "gz_create: %d\n", err); exit(1); }
  int q[192];
  for (int i = 0; i < 192; ++i) q[i] = 3;
  EXPECT(gz_encode_rgb(c, nullptr), GZ_OK);
  EXPECT(gz_quantize(c, q, nullptr), GZ_OK);
  const int cap = NB * 189;
  std::vector<int32_t> off(NB + 1);
  std::vector<uint8_t> idx(cap);
  std::vector<float> errs(cap);
  EXPECT(gz_block_zeroing_orders_masked(c, 7, 3, 1, off.data(), idx.data(), errs.data(), cap), GZ_OK);
  *candidates = (uint64_t)off[NB];
  if (reset) EXPECT(gz_order_reset(c), GZ_OK);
  float d = 0;
  EXPECT(gz_compare(c, &d, nullptr, nullptr), GZ_OK);
  return c;
}

static int fused_begin(gz_ctx* c, const int32_t* next_cand) {
  return gz_order_build_auto_descend_begin(c, 1, 1, 1.0, 1, next_cand, 0, 0.0f, PER_BLOCK, 16, LEVELS);
}

int main() {
  uint64_t candidates = 0, total = 0, below = 0, last = 0, exported = 0, log[3 * LEVELS];
  int32_t btc = 0;
  int levels = 0;
  float d = 0;
  void* mirror = nullptr;
  std::vector<int32_t> zero(NB, 0);

  // the fused iteration, twice: the second order's k_weights_gather makes the advance
  gz_ctx* c = searched(&candidates);
  EXPECT(gz_order_host_mirror(c, candidates, &mirror), GZ_OK);
  for (int it = 0; it < 2; ++it) {
    EXPECT(gz_compare_begin(c), GZ_OK);
    EXPECT(fused_begin(c, zero.data()), GZ_OK);
    EXPECT(gz_compare_end(c, &d), GZ_OK);
    EXPECT(gz_order_build_auto_end(c, &total, &btc, &below), GZ_OK);
    EXPECT(gz_order_descend_end(c, log, LEVELS, &levels, &last), GZ_OK);
    EXPECT(gz_order_exported(c, &exported), GZ_OK);
    if (total == 0 || total > candidates || levels < 1 || (it == 0 && exported == 0) || exported > total) {
      fprintf(stderr, "iteration %d: total %llu, levels %d, exported %llu\n", it, (unsigned long long)total, levels,
              (unsigned long long)exported);
      return 1;
    }
    std::vector<char> prefix((const char*)mirror, (const char*)mirror + 8 * exported);   // (reads what k_desc_export wrote)
    EXPECT(gz_order_advance(c, 0.25f, 1), GZ_OK);
  }
  EXPECT(gz_order_build_auto_end(c, &total, &btc, &below), GZ_E_STATE);   // a second end

  // a begin that supersedes a begin; then a synchronous build that supersedes both
  EXPECT(gz_compare_begin(c), GZ_OK);
  EXPECT(fused_begin(c, zero.data()), GZ_OK);
  EXPECT(fused_begin(c, zero.data()), GZ_OK);
  EXPECT(gz_order_build_auto_end(c, &total, &btc, &below), GZ_OK);
  EXPECT(gz_order_descend_end(c, log, LEVELS, &levels, &last), GZ_OK);
  EXPECT(gz_compare_end(c, &d), GZ_OK);
  EXPECT(fused_begin(c, zero.data()), GZ_OK);
  EXPECT(gz_order_build_auto(c, 1, 1, 1.0, 1, zero.data(), 0, 0.0f, &total, &btc, &below), GZ_OK);
  EXPECT(gz_order_build_auto_end(c, &total, &btc, &below), GZ_E_STATE);
  EXPECT(gz_order_descend_end(c, log, LEVELS, &levels, &last), GZ_OK);
  if (levels != 0) { fprintf(stderr, "a voided descent returned %d levels\n", levels); return 1; }

  // one failed launch (the order's fill), with a Compare pending: nothing of the call stays pending
  EXPECT(gz_compare_begin(c), GZ_OK);
  gz_emu_fail_launch(2);
  EXPECT(fused_begin(c, zero.data()), GZ_E_HIP);
  gz_emu_fail_launch(-1);
  EXPECT(gz_order_build_auto_end(c, &total, &btc, &below), GZ_E_STATE);
  EXPECT(gz_order_descend_end(c, log, LEVELS, &levels, &last), GZ_OK);
  EXPECT(gz_compare_end(c, &d), GZ_OK);
  if (levels != 0) { fprintf(stderr, "a failed begin left a descent of %d levels\n", levels); return 1; }

  // a new frame between begin and end
  EXPECT(gz_compare_begin(c), GZ_OK);
  EXPECT(fused_begin(c, zero.data()), GZ_OK);
  EXPECT(gz_set_frame(c, 2), GZ_OK);
  EXPECT(gz_order_build_auto_end(c, &total, &btc, &below), GZ_E_STATE);
  EXPECT(gz_order_descend_end(c, log, LEVELS, &levels, &last), GZ_OK);
  EXPECT(gz_compare_end(c, &d), GZ_E_STATE);
  EXPECT(gz_order_exported(c, &exported), GZ_OK);
  if (levels != 0 || exported != 0) { fprintf(stderr, "a new frame left %d levels, %llu exported\n", levels, (unsigned long long)exported); return 1; }
  gz_destroy(c);

  // out of memory inside a group made on first use (the order's block arrays, the entropy coder's buffers): the call
  // fails, the context stays valid, and the same call repeated makes the group in full
  c = searched(&candidates, false);
  uint64_t total2 = 0;
  gz_emu_fail_alloc(2);
  EXPECT(gz_order_build_auto(c, 1, 1, 1.0, 1, zero.data(), 0, 0.0f, &total, &btc, &below), GZ_E_NOMEM);
  gz_emu_fail_alloc(-1);
  EXPECT(gz_order_build_auto(c, 1, 1, 1.0, 1, zero.data(), 0, 0.0f, &total2, &btc, &below), GZ_OK);
  if (total2 == 0 || total2 > candidates) { fprintf(stderr, "the repeated order has %llu entries\n", (unsigned long long)total2); return 1; }
  int q[192];
  for (int i = 0; i < 192; ++i) q[i] = 3;
  std::vector<uint32_t> counts(1536), counts2(1536);
  gz_emu_fail_alloc(1);
  EXPECT(gz_jpeg_histograms(c, q, counts.data()), GZ_E_NOMEM);
  gz_emu_fail_alloc(-1);
  EXPECT(gz_jpeg_histograms(c, q, counts.data()), GZ_OK);
  EXPECT(gz_jpeg_histograms(c, q, counts2.data()), GZ_OK);
  if (counts != counts2 || counts[0] + counts[1] == 0) { fprintf(stderr, "the repeated histograms differ from the next ones\n"); return 1; }
  gz_destroy(c);
  printf("ok\n");
  return 0;
}
