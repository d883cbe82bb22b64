// uc_crest.hpp -- the crest rule of include/uchirp_align.h, once: the sinusoid through the three samples of one candidate,
// and the choice of the best candidate and its runner-up.  uc_align_peak, uc_xcorr_peak and uc_track_finish (which promise
// each other "the same bits") all go through these few lines: the floating-point operations and their order are the
// same by construction.  Which samples are candidates, NO_PEAK and AT_EDGE are the caller's business.  Host code only,
// header-only, in an anonymous namespace like uc_host.hpp; built with -ffp-contract=off like every host file.
#pragma once
#include <cmath>

namespace {

struct CrestFit {
  double height, d;   // the sinusoid's height, and its crest's offset from the middle sample, in samples
};

// the candidate with the samples (lo, mid, hi) = (r[k - 1], r[k], r[k + 1])
CrestFit crest_fit(double lo, double mid, double hi) {
  const double c = (lo + hi) / (2.0 * mid);
  CrestFit f = {mid, 0.0};
  if (c > -1.0 && c < 1.0) {
    const double w = std::acos(c);
    const double q = (hi - lo) / (2.0 * std::sin(w));
    f.height = std::hypot(mid, q);
    f.d = std::atan2(q, mid) / w;
  }
  return f;
}

// the candidates are added in ascending k; of equal heights the first one is the best
struct CrestChoice {
  double best = 0.0, second = 0.0, best_d = 0.0;
  int best_k = -1;   // -1: no candidate yet

  void add(int k, const CrestFit& f) {
    if (best_k < 0 || f.height > best) {
      if (best_k >= 0) second = best;
      best = f.height;
      best_d = f.d;
      best_k = k;
    } else if (f.height > second) {
      second = f.height;
    }
  }

  // into a peak record of uchirp_align.h / uchirp_xcorr.h / uchirp_track.h (one layout); needs best_k >= 0
  template <class Peak>
  void store(int max_lag, Peak* out) const {
    out->delay_samples = (double)(best_k - max_lag) + best_d;
    out->height = best;
    out->runner_up = second / best;
    out->lag = best_k - max_lag;
  }
};

}  // namespace
