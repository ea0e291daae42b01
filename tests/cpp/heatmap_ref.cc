// TEST ONLY (CPU): the reference's own heat map and fuzzy functions -- butteraugli::CreateHeatMapImage,
// ButteraugliFuzzyClass and ButteraugliFuzzyInverse (butteraugli.cc:1903-1992), as oracle/_ref/libgz_ref.so exports them
// -- behind a C interface for tests/test_heatmap_reference.py and tools/gen_heatmap_golden.py.  The three declarations
// are butteraugli.h's; nothing of the reference is compiled here.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace butteraugli {
double ButteraugliFuzzyClass(double score);
double ButteraugliFuzzyInverse(double seek);
void CreateHeatMapImage(const std::vector<float>& distmap, double good_threshold, double bad_threshold, size_t xsize, size_t ysize,
                        std::vector<uint8_t>* heatmap);
}  // namespace butteraugli

extern "C" {

// map: w * h floats, rows of w; out: w * h * 3 bytes
void ref_heatmap(const float* map, int w, int h, double good, double bad, uint8_t* out) {
  const std::vector<float> distmap(map, map + (size_t)w * h);
  std::vector<uint8_t> heat;
  butteraugli::CreateHeatMapImage(distmap, good, bad, (size_t)w, (size_t)h, &heat);
  memcpy(out, heat.data(), heat.size());
}

double ref_fuzzy_class(double score) { return butteraugli::ButteraugliFuzzyClass(score); }
double ref_fuzzy_inverse(double seek) { return butteraugli::ButteraugliFuzzyInverse(seek); }

}  // extern "C"
