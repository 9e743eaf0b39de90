// art_adaptive.h -- the per-pixel text of art_adaptive_estimate_device (include/art_hip.h states the arithmetic; this is its one
// definition).  ART_HD functions over plain pointers, no HIP types: art_adaptive.hip compiles them for gfx950 and tests/adaptive_host
// compiles the same text with g++ (the arrangement of art_temporal.h with tests/temporal_host), so the kernel and the host build cannot
// drift apart.
#pragma once
#include <math.h>
#include <stdint.h>
#include "art_hip.h"
#include "art_denoise.h"

namespace art {
namespace ad {

using dn::finite_f;

struct Params {
  int32_t n;                       // width * height
  int32_t per;                     // samples per colour: 4 with aa_on, else 1
  uint32_t min_colours, max_samples;
  float threshold, lum_floor;
};

// ArtAdaptiveParams and which pointers are given -> the kernel's Params: every refusal that needs no device.  Returns nullptr, or why the
// call is refused.  The library (art_device_entries.cpp) and tests/adaptive_host both derive their Params here.
inline const char* params_from_abi(const ArtAdaptiveParams* p, const void* accum3f, const void* moments2f, const void* counts1u, const void* mean3f,
                                   const void* variance1f, const void* error1f, const void* mask1b, Params& P) {
  if (!p) return "null ArtAdaptiveParams";
  if (!accum3f || !moments2f || !counts1u) return "null accum3f, moments2f or counts1u";
  if (!mean3f && !variance1f && !error1f && !mask1b) return "no output is wanted (all four pointers are null)";
  if (p->width < 1 || p->height < 1 || (int64_t)p->width * p->height > (1ll << 28)) return "width and height must be at least 1 and width * height at most 2^28";
  if (p->min_colours < 2) return "min_colours must be at least 2";
  if (p->max_samples < 0) return "max_samples must not be negative";
  if (p->threshold != p->threshold) return "threshold is NaN";
  if (!finite_f(p->lum_floor) || p->lum_floor < 0.0f) return "lum_floor must be finite and not negative";
  P.n = p->width * p->height; P.per = p->aa_on ? 4 : 1;
  P.min_colours = (uint32_t)p->min_colours; P.max_samples = (uint32_t)p->max_samples;
  P.threshold = p->threshold; P.lum_floor = p->lum_floor;
  return nullptr;
}

struct Out { float mean[3]; float variance, error; uint8_t mask; };

// pixel q: the mean colour, the variance of the mean's luminance, the relative error and whether the next masked pass takes the pixel
ART_HD Out adaptive_pixel(const Params& P, const float* accum, const float* moments, const uint32_t* counts, size_t q) {
  const float inf = __builtin_bit_cast(float, 0x7f800000u);
  const uint32_t s = counts[q];
  Out o;
  o.mean[0] = o.mean[1] = o.mean[2] = 0.0f; o.variance = inf; o.error = inf;
  const double n = (double)s / (double)P.per, k = 1.0 / (double)P.per;
  if (s != 0u) {
    const float r = 1.0f / (float)s;
    o.mean[0] = r * accum[3 * q]; o.mean[1] = r * accum[3 * q + 1]; o.mean[2] = r * accum[3 * q + 2];
    if (!(n < 2.0)) {
      const double S1 = (double)moments[2 * q], S2 = (double)moments[2 * q + 1];
      const double D = S2 - (S1 * S1) / n;
      const double D0 = (D < 0.0) ? 0.0 : D;
      const double v = (D0 * (n / (n - 1.0))) / n;
      const double m = (S1 / n) * k;
      o.variance = (float)(v * (k * k));
      o.error = (float)((sqrt(v) * k) / (fabs(m) + (double)P.lum_floor));
      // a NaN leaves as THE quiet NaN: which sign and payload an operation gives a NaN differs between processors (x86 keeps an operand's,
      // gfx950 negates it with the subtrahend), and the contract is bit for bit
      const float qnan = __builtin_bit_cast(float, 0x7fc00000u);
      if (o.variance != o.variance) o.variance = qnan;
      if (o.error != o.error) o.error = qnan;
    }
  }
  o.mask = (s < P.max_samples && (n < (double)P.min_colours || !(o.error <= P.threshold))) ? 1 : 0;
  return o;
}

}  // namespace ad

// ---- launch interface (art_adaptive.hip); hipcc only: the g++ builds of the tests take the per-pixel text above and nothing else
#if defined(__HIPCC__)
// art_adaptive_estimate_device (art_adaptive.hip, art_device_entries.cpp adaptive_estimate_device): the caller's planes, outputs nullptr where not wanted
struct AdaptiveArgs {
  ad::Params P;
  const float* accum; const float* moments; const uint32_t* counts;
  float* mean; float* variance; float* error; uint8_t* mask;
};
void launch_adaptive_estimate(hipStream_t st, const AdaptiveArgs& A);
#endif

}  // namespace art
