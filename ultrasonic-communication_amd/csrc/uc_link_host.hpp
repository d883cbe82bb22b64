// uc_link_host.hpp -- what the C-ABI files of libuchirp_link.so (uc_link_api.cpp) and libuchirp_scene.so
// (uc_scene_api.cpp) share on top of uc_host.hpp: the checks and defaults of the frame format and of the output formats.
// The RESTRICTION of uc_host.hpp (one including translation unit per library) holds for this header too.
#pragma once
#include "uc_host.hpp"

#include "../../include/uchirp_link.h"

namespace {

bool is_device_ptr(const void* p) { return device_of(p) >= 0; }

size_t elem_size(int dtype) {
  switch (dtype) {
    case UC_LINK_DTYPE_I32:
    case UC_LINK_DTYPE_F32: return 4;
    case UC_LINK_DTYPE_I16: return 2;
    default: return 0;
  }
}

bool config_ok(const uc_link_config* c) {
  if (!(c->fs_tx > 0.0) || !(c->t_symbol > 0.0) || !std::isfinite(c->fs_tx) || !std::isfinite(c->t_symbol)) return false;
  if (!std::isfinite(c->f0) || !std::isfinite(c->f1)) return false;
  const double n = c->t_symbol * c->fs_tx;
  return n >= 2.0 && n < 1e9 && c->n_preamble < (1u << 20) && c->n_guard < (1u << 20);
}

// a + b = s + e exactly (Knuth)
inline void two_sum(double a, double b, double& s, double& e) {
  s = a + b;
  const double bb = s - a;
  e = (a - (s - bb)) + (b - bb);
}

// What the kernels take a stream's (a path's) time from: the seconds since the frame began at absolute sample j are
//   tt = (j - origin) * rate + t0
// origin: the integer nearest to lead_samples / (1 + ppm * 1e-6), where the frame begins on the receiver's clock, held to
//         +-2^53 (a frame that begins further off begins after every sample the calls accept, or began before sample
//         -2^53; frame_time()'s monotonicity needs |j - origin| < 2^54);
// t0:     (origin * (1 + ppm * 1e-6) - lead_samples) / fs_out, the frame's time at that sample: under a sample in size, but
//         the difference of two numbers as large as the lead.  It is summed in pairs of doubles: ppm / 10^6 as hi + lo
//         (lo from the division's exact remainder, so 1e-6 here is the number 10^-6 and not its double), origin * hi with
//         its fma remainder, origin - lead and the sum of the two large parts with their two_sum remainders.  Every remainder is
//         exact, so what is rounded are terms of the size of the result: t0 is within 2 ulp of the rational value for
//         |ppm| <= 200 and |lead| <= 2^53 (tests/test_far_cpu.py holds it against fractions);
// rate:   (1 / fs_out) * (1 + ppm * 1e-6) in double as before: 3 roundings, times the seconds INSIDE a frame only.
// Every double operation here is IEEE and unfused (this file is compiled with -ffp-contract=off; fma is the call).
struct FrameOrigin {
  int64_t origin;
  double t0, rate;
};

FrameOrigin frame_origin(double lead_samples, float ppm, double fs_out) {
  const double pp = (double)ppm;
  const double e_hi = pp / 1e6;
  const double e_lo = std::fma(-e_hi, 1e6, pp) / 1e6;
  double q = lead_samples / (1.0 + e_hi);
  if (!(q == q)) q = 0.0;                                  // 0 / 0: ppm = -10^6 and no lead
  q = std::fmin(std::fmax(q, -0x1p53), 0x1p53);
  const double jd = std::nearbyint(q);                     // to nearest, ties to even; exact in double
  double d, d_err, s, s_err;
  two_sum(jd, -lead_samples, d, d_err);
  const double p = jd * e_hi, p_err = std::fma(jd, e_hi, -p);
  two_sum(d, p, s, s_err);
  const double u = s + (((s_err + p_err) + jd * e_lo) + d_err);
  FrameOrigin o;
  o.origin = (int64_t)jd;
  o.t0 = u / fs_out;
  o.rate = (1.0 / fs_out) * (1.0 + pp * 1e-6);
  return o;
}

// the format of the reference transmission: 44100 Hz, 0.0262 s, 16000 .. 19000 Hz, 7 preamble symbols, 12 guard symbols
void reference_config(uc_link_config* cfg) {
  memset(cfg, 0, sizeof(*cfg));
  cfg->fs_tx = 44100.0;
  cfg->t_symbol = 0.0262;
  cfg->f0 = 16000.0;
  cfg->f1 = 19000.0;
  cfg->n_preamble = 7;
  cfg->n_guard = 12;
}

}  // namespace
