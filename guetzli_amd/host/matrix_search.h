// The quant-matrix bisection of the host search driver: pure logic, no device calls.
// QuantMatrixGenerator (processor.cc:194-296): a 1-D family of matrices indexed by a
// "heuristic score"; bracket a passing (a) and a failing (b) score, then bisect.
#pragma once
#include <string.h>

#include <algorithm>
#include <vector>

#include "jpeg_writer.h"

namespace guetzli_amd {

typedef int QuantMatrix[3][64];

inline double Csf(int k) { return 1.0 / (1.0 + kZigZagOrder[k] / 2.0); }

inline double HeuristicScore(const QuantMatrix q) {   // QuantMatrixHeuristicScore, :182-190
  double score = 0.0;
  for (int c = 0; c < 3; ++c)
    for (int k = 0; k < 64; ++k) score += 0.5 * (q[c][k] - 1.0) * Csf(k);
  return score;
}

inline bool SameMatrix(const QuantMatrix a, const QuantMatrix b) {
  return memcmp(a, b, sizeof(QuantMatrix)) == 0;
}

struct Trial {
  QuantMatrix q;
  size_t jpg_size;
  bool dist_ok;
};

class MatrixSearch {
 public:
  explicit MatrixSearch(bool downsample) : downsample_(downsample), lo_(-1.0), hi_(-1.0), total_(0.0) {
    for (int k = 0; k < 64; ++k) total_ += 3.0 * Csf(k);
  }
  bool Next(QuantMatrix q) {
    for (int guard = 0; guard < 1000; ++guard) {
      double h;
      if (hi_ == -1.0) {
        if (lo_ == -1.0) {
          h = downsample_ ? 0.0 : total_;
        } else {
          h = lo_ < 5.0 * total_ ? lo_ + total_ : 2 * (lo_ + total_);
        }
        if (h > 100 * total_) return false;   // nothing creates enough error
      } else if (hi_ == 0.0) {
        return false;
      } else if (lo_ == -1.0) {
        h = 0.0;
      } else {
        QuantMatrix lower, upper;
        const double eps = 0.05;
        FromScore((1 - eps) * lo_ + eps * 0.5 * (lo_ + hi_), lower);
        FromScore((1 - eps) * hi_ + eps * 0.5 * (lo_ + hi_), upper);
        if (SameMatrix(lower, upper)) return false;
        h = (lo_ + hi_) * 0.5;
      }
      FromScore(h, q);
      bool seen = false;
      for (size_t i = 0; i < tried_.size(); ++i) {
        if (SameMatrix(q, tried_[i].q)) {
          if (tried_[i].dist_ok) lo_ = h; else hi_ = h;
          seen = true;
          break;
        }
      }
      if (!seen) return true;
    }
    return false;
  }
  void Add(const Trial& t) {
    tried_.push_back(t);
    const double h = HeuristicScore(t.q);
    if (t.dist_ok) lo_ = std::max(lo_, h);
    else hi_ = hi_ == -1.0 ? h : std::min(hi_, h);
  }

 private:
  void FromScore(double score, QuantMatrix q) const {   // :269-279
    const int level = static_cast<int>(score / total_);
    score -= level * total_;
    for (int k = 63; k >= 0; --k) {
      const int nat = kNaturalOrder[k];
      for (int c = 0; c < 3; ++c) q[c][nat] = 2 * level + (score > 0.0 ? 3 : 1);
      score -= 3.0 * Csf(nat);
    }
  }
  const bool downsample_;
  double lo_, hi_, total_;
  std::vector<Trial> tried_;
};

}  // namespace guetzli_amd
