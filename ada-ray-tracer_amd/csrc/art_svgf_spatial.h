// art_svgf_spatial.h -- the per-pixel text of art_svgf_spatial_variance_device (include/art_hip.h states the arithmetic; this is its one
// definition).  ART_HD functions over plain pointers, no HIP types: art_svgf_spatial.hip compiles them for gfx950 and
// tests/svgf_spatial_host compiles the same text with g++ (the arrangement of art_temporal.h with tests/temporal_host), so the kernel and
// the host build cannot drift apart.
//
// The history is art_temporal_device's hist_out (art_temporal.h): three planes of 16-byte records, so a tap costs three 16-byte loads.
// The stops are the a-trous filters' own (dn::stop_weight, art_denoise.h), with no spline weight and no colour term.
#pragma once
#include <stdint.h>
#include "art_hip.h"
#include "art_denoise.h"

namespace art {
namespace sv {

using dn::Rec4;
using dn::finite_f;

struct Params {
  int32_t W, H;
  int32_t radius, normal_log2;
  float min_history, sigma_depth;
};

// ArtSvgfSpatialParams and the pointers -> the kernel's Params: every refusal that needs no device.  Returns nullptr, or why the call is
// refused.  The library (art_device_entries.cpp) and tests/svgf_spatial_host both derive their Params here.
inline const char* params_from_abi(const ArtSvgfSpatialParams* p, const void* hist, const void* variance_in1f, const void* variance_out1f, Params& P) {
  if (!p) return "null ArtSvgfSpatialParams";
  if (!hist || !variance_in1f || !variance_out1f) return "null hist, variance_in1f or variance_out1f";
  if (p->width < 1 || p->height < 1 || (int64_t)p->width * p->height > (1ll << 28)) return "width and height must be at least 1 and width * height at most 2^28";
  if (p->radius < 1 || p->radius > 3) return "radius must be 1 .. 3";
  if (p->normal_log2 < 0 || p->normal_log2 > 10) return "normal_log2 must be 0 .. 10";
  if (p->min_history != p->min_history || p->sigma_depth != p->sigma_depth) return "min_history or sigma_depth is NaN";
  const size_t N = (size_t)p->width * (size_t)p->height;
  const char* h = (const char*)hist; const char* o = (const char*)variance_out1f;
  if (o < h + 48 * N && h < o + 4 * N) return "variance_out1f overlaps hist";
  P.W = p->width; P.H = p->height; P.radius = p->radius; P.normal_log2 = p->normal_log2;
  P.min_history = p->min_history; P.sigma_depth = p->sigma_depth;
  return nullptr;
}

// a pixel with a long history keeps its word of variance_in: n is plane 0's fourth word, v the pixel's variance_in
ART_HD bool long_history(const Params& P, float n, float v) { return n >= P.min_history && finite_f(v); }

// a pixel with a short history at (x, y): the variance of its mean luminance from the moments pooled over the window
ART_HD float pooled_variance(const Params& P, const Rec4* hist, int x, int y) {
  const size_t N = (size_t)P.W * (size_t)P.H;
  const size_t p = (size_t)y * (size_t)P.W + (size_t)x;
  const float n_p = hist[p].w;
  const Rec4 bp = hist[N + p], cp = hist[2 * N + p];
  dn::Stops stops = {mk3(cp.x, cp.y, cp.z), 1, P.normal_log2, P.sigma_depth > 0.0f, bp.z, 0.0f, 0.0f, 1e-3f * bp.z + 1e-6f, P.sigma_depth};
  if (stops.use_depth) dn::central_difference(P.W, P.H, x, y, [hist, N](size_t k) { return hist[N + k].z; }, stops.gx, stops.gy);
  double Ns = 0.0, S1 = 0.0, S2 = 0.0;
  for (int dy = -P.radius; dy <= P.radius; ++dy) {
    const int qy = y + dy;
    if (qy < 0 || qy >= P.H) continue;
    for (int dx = -P.radius; dx <= P.radius; ++dx) {
      const int qx = x + dx;
      if (qx < 0 || qx >= P.W) continue;
      const size_t q = (size_t)qy * (size_t)P.W + (size_t)qx;
      const float nq = hist[q].w;
      if (!(finite_f(nq) && nq > 0.0f)) continue;
      const Rec4 b = hist[N + q];
      if (!(finite_f(b.x) && finite_f(b.y) && finite_f(b.z))) continue;
      const Rec4 c = hist[2 * N + q];
      if (!(finite_f(c.x) && finite_f(c.y) && finite_f(c.z))) continue;
      float w = 1.0f;
      if ((dx != 0 || dy != 0) && !dn::stop_weight(stops, 1.0f, mk3(c.x, c.y, c.z), b.z, (float)dx, (float)dy, 0.0f, w)) continue;
      const double k = (double)w * (double)nq;
      Ns += k; S1 += k * (double)b.x; S2 += k * (double)b.y;
    }
  }
  if (Ns < 2.0) return __builtin_bit_cast(float, 0x7f800000u);
  const double M1 = S1 / Ns, M2 = S2 / Ns;
  const double D = M2 - M1 * M1;
  const float v = (float)((((D < 0.0) ? 0.0 : D) * (Ns / (Ns - 1.0))) / (double)n_p);
  // a NaN leaves as THE quiet NaN (art_adaptive.h: processors differ in the sign and payload they give one)
  return (v != v) ? __builtin_bit_cast(float, 0x7fc00000u) : v;
}

// pixel (x, y) of the frame: its word of variance_out
ART_HD float spatial_pixel(const Params& P, const Rec4* hist, const float* variance_in, int x, int y) {
  const size_t p = (size_t)y * (size_t)P.W + (size_t)x;
  const float v = variance_in[p];
  if (long_history(P, hist[p].w, v)) return v;
  return pooled_variance(P, hist, x, y);
}

}  // namespace sv

// ---- launch interface (art_svgf_spatial.hip); hipcc only: the g++ builds of the tests take the per-pixel text above and nothing else
#if defined(__HIPCC__)
// art_svgf_spatial_variance_device (art_svgf_spatial.hip, art_device_entries.cpp svgf_spatial_variance_device): the history of art_temporal_device and
// the caller's two variance planes (they may be one); tiles_x = svgf_spatial_tiles_x(P.W), the kernel's tiles per row of tiles
struct SvgfSpatialArgs {
  sv::Params P;
  int32_t tiles_x;
  const sv::Rec4* hist; const float* variance_in; float* variance_out;
};
int svgf_spatial_tiles_x(int width);
void launch_svgf_spatial(hipStream_t st, const SvgfSpatialArgs& A);
#endif

}  // namespace art
