// art_denoise.h -- the per-pixel text of art_denoise_device, art_denoise_svgf_device and art_denoise_svgf_var_device (include/art_hip.h
// states the arithmetic; this is its one definition): one tap weight, one tap loop, one preparation, and the refusals of their arguments.
// ART_HD functions over plain pointers, no HIP types: art_denoise.hip compiles them for gfx950 and tests/denoise_host, tests/svgf_host
// and tests/temporal_host compile the same text with g++ (the arrangement of art_shade.h with tests/host_sim), so the kernels and the
// host builds cannot drift apart.
//
// Working data of art_denoise_device (the library's scratch, one entry per pixel, row-major; the other two: dn::Mode below):
//   image   Rec4 {r, g, b, z}         c_i and the pixel's depth (0 without a depth plane); two of them, read and written in turn
//   guide   Rec4 {nx, ny, nz, flags}  the normal ((0, 0, 0) without a normal plane) and, as a word, bit 0 = bad in guides; constant over the iterations
//   grad    Rec2 {gx, gy}             the depth gradient, read for the centre only
// so a tap costs two 16-byte loads.  "Bad in colour" follows c_i (a repaired pixel is good in the next iteration) and is read off the
// tap's own colour.
#pragma once
#include "art_hip.h"
#include "art_math.h"

namespace art {
namespace dn {

struct alignas(16) Rec4 { float x, y, z, w; };
struct alignas(8) Rec2 { float x, y; };

struct Params {
  int32_t W, H;
  int32_t normal_log2;
  int32_t demod;                   // demodulate != 0 and an albedo plane is given
  int32_t has_normal, has_depth;
  float scale, sigma_color, sigma_depth;
};

constexpr uint32_t kBadGuides = 1u;

ART_HD bool finite_f(float v) { return (__builtin_bit_cast(uint32_t, v) & 0x7f800000u) != 0x7f800000u; }
ART_HD bool finite_rgb(const Rec4& c) { return finite_f(c.x) && finite_f(c.y) && finite_f(c.z); }
ART_HD float lum(const Rec4& c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }
ART_HD float spline(int a) { return a == 0 ? 0.375f : (a == 1 || a == -1) ? 0.25f : 0.0625f; }
ART_HD float albedo_floor(float a) { return amax(a, 1e-3f); }

// the clamped central difference of a plane at (x, y); f(k) is the plane's value at the linear index k
template <class F>
ART_HD void central_difference(int W, int H, int x, int y, F f, float& gx, float& gy) {
  const int x1 = (x + 1 < W) ? x + 1 : W - 1, x0 = (x > 0) ? x - 1 : 0;
  const int y1 = (y + 1 < H) ? y + 1 : H - 1, y0 = (y > 0) ? y - 1 : 0;
  const size_t row = (size_t)y * (size_t)W;
  gx = 0.5f * (f(row + (size_t)x1) - f(row + (size_t)x0));
  gy = 0.5f * (f((size_t)y1 * (size_t)W + (size_t)x) - f((size_t)y0 * (size_t)W + (size_t)x));
}

// preparation of pixel (x, y): c_0, the guide record and the depth gradient
ART_HD void pack_pixel(const Params& P, const float* color, const float* albedo, const float* normal, const float* depth, int x, int y,
                       Rec4& c, Rec4& g, Rec2& d) {
  const size_t p = (size_t)y * (size_t)P.W + (size_t)x;
  c.x = P.scale * color[3 * p]; c.y = P.scale * color[3 * p + 1]; c.z = P.scale * color[3 * p + 2]; c.w = 0.0f;
  if (P.demod) {
    c.x = c.x / albedo_floor(albedo[3 * p]); c.y = c.y / albedo_floor(albedo[3 * p + 1]); c.z = c.z / albedo_floor(albedo[3 * p + 2]);
  }
  uint32_t flags = 0;
  g.x = g.y = g.z = 0.0f;
  if (P.has_normal) {
    g.x = normal[3 * p]; g.y = normal[3 * p + 1]; g.z = normal[3 * p + 2];
    if (!(finite_f(g.x) && finite_f(g.y) && finite_f(g.z))) flags |= kBadGuides;
  }
  d.x = d.y = 0.0f;
  if (P.has_depth) {
    c.w = depth[p];
    if (!finite_f(c.w)) flags |= kBadGuides;
    central_difference(P.W, P.H, x, y, [depth](size_t k) { return depth[k]; }, d.x, d.y);
  }
  g.w = __builtin_bit_cast(float, flags);
}

// The edge-stopping weight of a tap other than the centre, the one text of it: the a-trous filters below and sv::pooled_variance
// (art_svgf_spatial.h) all call it.  Stops holds what a centre's taps share.
struct Stops {
  f3 n;                            // the centre's normal
  int32_t has_normal, normal_log2;
  bool use_depth;
  float z, gx, gy, zfloor;         // the centre's depth, its depth gradient and the floor of the depth stop's divisor
  float sigma_depth;
};

// w = (h * wn) * e for the tap at offset (ox, oy) pixels with normal nq and depth zq (read only with use_depth); h is the tap's spline
// weight (1.0f where there is none: 1.0f * wn is wn) and xc the colour term, which the caller computes (0 when it is off).  Returns
// false when the tap is to be skipped: the argument of the exponential is NaN or positive (a negative depth), or a weight is NaN.
ART_HD bool stop_weight(const Stops& c, float h, const f3& nq, float zq, float ox, float oy, float xc, float& w) {
  float wn = 1.0f;
  if (c.has_normal) {
    wn = amax(dot(c.n, nq), 0.0f);
    for (int j = 0; j < c.normal_log2; ++j) wn = wn * wn;
  }
  float xz = 0.0f;
  if (c.use_depth) xz = fabsf(c.z - zq) / (c.sigma_depth * (fabsf(c.gx * ox) + fabsf(c.gy * oy)) + c.zfloor);
  const double t = -((double)xz + (double)xc);
  float e;
  if (t < -200.0) e = 0.0f;
  else if (t <= 0.0) e = (float)m1::exp_small(t);
  else e = __builtin_bit_cast(float, 0x7fc00000u);        // t NaN or positive: w is NaN
  w = (h * wn) * e;
  return w == w;
}

// after the last iteration: the output of pixel p
ART_HD void finish_pixel(const Params& P, const float* albedo, size_t p, const Rec4& c, float& r, float& g, float& b) {
  r = c.x; g = c.y; b = c.z;
  if (P.demod) { r = r * albedo_floor(albedo[3 * p]); g = g * albedo_floor(albedo[3 * p + 1]); b = b * albedo_floor(albedo[3 * p + 2]); }
}

// ---- the three entries: one preparation each, and two filters ------------------------------------------------------------------
// art_denoise_svgf_device and art_denoise_svgf_var_device (include/art_hip.h states their arithmetic) carry a variance through the
// filter.  Their working data, one entry per pixel, row-major:
//   image   Rec4 {r, g, b, v}         c_i and v_i, the variance of the pixel's luminance estimate; two of them, read and written in turn
//   guide   Rec4 {nx, ny, nz, flags}  as above, plus bit 1 = no colour stop when this pixel is the centre (its v was not finite)
//   z       float                     the depth, a plane of its own: read for a tap only when the depth stop is on
//   grad    Rec2 {gx, gy}             as above
// so a tap costs two 16-byte loads and, with a depth plane, one dword load; the variance prefilter reads the same two records of the
// centre's 3 x 3 neighbours.
enum class Mode { Plain, Svgf, SvgfVar };      // art_denoise_device | v_0 from the luminance moments | v_0 from a variance plane
constexpr bool carries_variance(Mode m) { return m != Mode::Plain; }
constexpr uint32_t kNoColourStop = 2u;

ART_HD float lum3(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// v, the variance of pixel p's luminance estimate in the units of the colour plane, to v_0: scaled, demodulated, and stored in c.w
ART_HD void variance_to_v0(const Params& P, const float* albedo, size_t p, double v, Rec4& c, Rec4& g) {
  v = v * ((double)P.scale * (double)P.scale);
  if (P.demod) {
    const double la = (double)lum3(albedo_floor(albedo[3 * p]), albedo_floor(albedo[3 * p + 1]), albedo_floor(albedo[3 * p + 2]));
    v = v / (la * la);
  }
  c.w = (float)v;
  if (!finite_f(c.w)) {
    c.w = 0.0f;
    g.w = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, g.w) | kNoColourStop);
  }
}

// preparation of pixel (x, y) with v_0 from the moments: pack_pixel's c_0, guide record and gradient, the depth on its own, and the variance
// of the mean luminance of n_colours colours in binary64
ART_HD void svgf_pack_pixel(const Params& P, int32_t n_colours, const float* color, const float* moments, const float* albedo, const float* normal,
                            const float* depth, int x, int y, Rec4& c, Rec4& g, float& z, Rec2& d) {
  pack_pixel(P, color, albedo, normal, depth, x, y, c, g, d);
  z = c.w;
  const size_t p = (size_t)y * (size_t)P.W + (size_t)x;
  const double n = (double)n_colours;
  const double s1 = (double)moments[2 * p], s2 = (double)moments[2 * p + 1];
  const double D = s2 - (s1 * s1) / n;
  variance_to_v0(P, albedo, p, ((D < 0.0) ? 0.0 : D) * (n / (n - 1.0)), c, g);
}

// the same preparation with v_0 from a variance plane (one float per pixel) instead of the moments
ART_HD void svgf_var_pack_pixel(const Params& P, const float* color, const float* variance, const float* albedo, const float* normal,
                                const float* depth, int x, int y, Rec4& c, Rec4& g, float& z, Rec2& d) {
  pack_pixel(P, color, albedo, normal, depth, x, y, c, g, d);
  z = c.w;
  const size_t p = (size_t)y * (size_t)P.W + (size_t)x;
  variance_to_v0(P, albedo, p, (double)variance[p], c, g);
}

// the preparation of mode M, for the code that is written once over the modes (the pack kernel, the host driver under tests/): `moments`
// is the moments plane or, for SvgfVar, the variance plane; Plain reads neither it nor n_colours and leaves z alone
template <Mode M>
ART_HD void prepare_pixel(const Params& P, int32_t n_colours, const float* color, const float* moments, const float* albedo, const float* normal,
                          const float* depth, int x, int y, Rec4& c, Rec4& g, float& z, Rec2& d) {
  if constexpr (M == Mode::Plain) pack_pixel(P, color, albedo, normal, depth, x, y, c, g, d);
  else if constexpr (M == Mode::Svgf) svgf_pack_pixel(P, n_colours, color, moments, albedo, normal, depth, x, y, c, g, z, d);
  else svgf_var_pack_pixel(P, color, moments, albedo, normal, depth, x, y, c, g, z, d);
}

// the variance prefilter at (x, y): 3 x 3 at spacing 1 over the taps that are inside, good in guides and finite in colour
ART_HD float prefiltered_variance(const Params& P, const Rec4* image, const Rec4* guide, int x, int y) {
  float vs = 0.0f, ks = 0.0f;
  for (int dy = -1; dy <= 1; ++dy) {
    const int qy = y + dy;
    if (qy < 0 || qy >= P.H) continue;
    for (int dx = -1; dx <= 1; ++dx) {
      const int qx = x + dx;
      if (qx < 0 || qx >= P.W) continue;
      const size_t q = (size_t)qy * (size_t)P.W + (size_t)qx;
      if (__builtin_bit_cast(uint32_t, guide[q].w) & kBadGuides) continue;
      const Rec4 cq = image[q];
      if (!finite_rgb(cq)) continue;
      const float k = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);
      vs += k * cq.w; ks += k;
    }
  }
  return (ks > 0.0f) ? vs / ks : 0.0f;
}

// iteration i at centre (x, y).  VARIANCE (the two Svgf modes): {c_{i+1}, v_{i+1}}, the depth from zplane, the colour stop in standard
// deviations of the prefiltered variance.  Without it: c_{i+1} with the centre's depth carried along in .w; zplane is not read.
template <bool VARIANCE>
ART_HD Rec4 atrous_pixel(const Params& P, const Rec4* image, const Rec4* guide, const float* zplane, const Rec2* grad, int x, int y, int i) {
  const int s = 1 << i;
  const size_t p = (size_t)y * (size_t)P.W + (size_t)x;
  const Rec4 cp = image[p], gp = guide[p];
  const Rec2 dp = grad[p];
  bool use_colour = P.sigma_color > 0.0f && finite_rgb(cp);
  float zp, sc;
  if constexpr (VARIANCE) {
    zp = P.has_depth ? zplane[p] : 0.0f;
    use_colour = use_colour && !(__builtin_bit_cast(uint32_t, gp.w) & kNoColourStop);
    sc = P.sigma_color * sqrtf(prefiltered_variance(P, image, guide, x, y)) + 1e-6f;
  } else {
    zp = cp.w;
    sc = P.sigma_color * __builtin_bit_cast(float, (uint32_t)(127 - i) << 23);      // sigma_color * 2^-i
  }
  const float lp = lum(cp);
  const Stops stops = {mk3(gp.x, gp.y, gp.z), P.has_normal, P.normal_log2, P.has_depth && P.sigma_depth > 0.0f, zp, dp.x, dp.y, 1e-3f * zp + 1e-6f, P.sigma_depth};
  float ar = 0.0f, ag = 0.0f, ab = 0.0f, av = 0.0f, wsum = 0.0f;
  for (int dy = -2; dy <= 2; ++dy) {
    const int qy = y + s * dy;
    if (qy < 0 || qy >= P.H) continue;
    for (int dx = -2; dx <= 2; ++dx) {
      const int qx = x + s * dx;
      if (qx < 0 || qx >= P.W) continue;
      const size_t q = (size_t)qy * (size_t)P.W + (size_t)qx;
      const Rec4 gq = guide[q];
      if (__builtin_bit_cast(uint32_t, gq.w) & kBadGuides) continue;
      const Rec4 cq = image[q];
      if (!finite_rgb(cq)) continue;
      float w = spline(dx) * spline(dy);
      if (dx != 0 || dy != 0) {
        float zq = cq.w;
        if constexpr (VARIANCE) zq = stops.use_depth ? zplane[q] : 0.0f;
        const float xc = use_colour ? fabsf(lp - lum(cq)) / sc : 0.0f;
        if (!stop_weight(stops, w, mk3(gq.x, gq.y, gq.z), zq, (float)(s * dx), (float)(s * dy), xc, w)) continue;
      }
      ar += w * cq.x; ag += w * cq.y; ab += w * cq.z;
      if constexpr (VARIANCE) av += (w * w) * cq.w;
      wsum += w;
    }
  }
  Rec4 r = cp;
  if (wsum > 0.0f) {
    r.x = ar / wsum; r.y = ag / wsum; r.z = ab / wsum;
    if constexpr (VARIANCE) r.w = av / (wsum * wsum);
  }
  return r;
}

// the two filters by name: art_denoise_device's, which has no z plane, and the variance-guided one
ART_HD Rec4 atrous_pixel(const Params& P, const Rec4* image, const Rec4* guide, const Rec2* grad, int x, int y, int i) {
  return atrous_pixel<false>(P, image, guide, nullptr, grad, x, y, i);
}
ART_HD Rec4 svgf_atrous_pixel(const Params& P, const Rec4* image, const Rec4* guide, const float* zplane, const Rec2* grad, int x, int y, int i) {
  return atrous_pixel<true>(P, image, guide, zplane, grad, x, y, i);
}

// ---- the ABI's parameters and the pointers -> Params: every refusal that needs no device.  Each returns nullptr, or why the call is
// refused.  The library (art_device_entries.cpp) and the host builds under tests/ both derive their Params here.
template <class Abi>      // ArtDenoiseParams or ArtSvgfParams: what the two have in common
inline const char* frame_refusal(const Abi* p) {
  if (p->width < 1 || p->height < 1 || (int64_t)p->width * p->height > (1ll << 28)) return "width and height must be at least 1 and width * height at most 2^28";
  if (p->iterations < 1 || p->iterations > 8) return "iterations must be 1 .. 8";
  if (p->normal_log2 < 0 || p->normal_log2 > 10) return "normal_log2 must be 0 .. 10";
  return nullptr;
}
template <class Abi>
inline const char* fill_params(const Abi* p, const void* albedo3f, const void* normal3f, const void* depth, Params& P) {
  if (!finite_f(p->scale)) return "scale is not finite";
  if (p->sigma_color != p->sigma_color || p->sigma_depth != p->sigma_depth) return "a sigma is NaN";
  P.W = p->width; P.H = p->height; P.normal_log2 = p->normal_log2; P.demod = (p->demodulate != 0 && albedo3f) ? 1 : 0;
  P.has_normal = normal3f ? 1 : 0; P.has_depth = depth ? 1 : 0;
  P.scale = p->scale; P.sigma_color = p->sigma_color; P.sigma_depth = p->sigma_depth;
  return nullptr;
}

inline const char* params_from_abi(const ArtDenoiseParams* p, const void* color3f, const void* albedo3f, const void* normal3f, const void* depth, const void* out3f, Params& P) {
  if (!p) return "null ArtDenoiseParams";
  if (!color3f || !out3f) return "null color3f or out3f";
  if (const char* why = frame_refusal(p)) return why;
  if (p->variant < 0 || p->variant > 2) return "variant must be 0 .. 2";
  return fill_params(p, albedo3f, normal3f, depth, P);
}

// variance_plane: art_denoise_svgf_var_device, whose `moments` is the variance plane and which does not read n_colours
inline const char* params_from_abi(const ArtSvgfParams* p, const void* color3f, const void* moments, const void* albedo3f, const void* normal3f, const void* depth,
                                   const void* out3f, bool variance_plane, Params& P) {
  if (!p) return "null ArtSvgfParams";
  if (!color3f || !out3f) return "null color3f or out3f";
  if (!moments) return variance_plane ? "null variance1f" : "null moments2f";
  if (const char* why = frame_refusal(p)) return why;
  if (!variance_plane && p->n_colours < 2) return "n_colours must be at least 2";
  return fill_params(p, albedo3f, normal3f, depth, P);
}

}  // namespace dn

// ---- launch interface (art_denoise.hip); hipcc only: the g++ builds of the tests take the per-pixel text above and nothing else
#if defined(__HIPCC__)
// art_denoise_device, art_denoise_svgf_device and art_denoise_svgf_var_device (art_denoise.hip, art_device_entries.cpp run_denoise): the caller's planes
// (albedo / normal / depth / variance_out nullptr: not given; out may be color) and the library's scratch records of art_denoise.h, n = W * H
// of each.  moments: the moments plane or, for dn::Mode::SvgfVar, the variance plane (n_colours is then not read).  dn::Mode::Plain leaves
// n_colours, moments, variance_out and z zero: its kernels read none of them.
struct DenoiseArgs {
  dn::Params P;
  int32_t n, n_colours;
  const float* color; const float* moments; const float* albedo; const float* normal; const float* depth;
  float* out; float* variance_out;
  dn::Rec4* image[2]; dn::Rec4* guide; float* z; dn::Rec2* grad;
};
void launch_denoise(hipStream_t st, dn::Mode mode, const DenoiseArgs& A, int iterations);      // the mode's pack kernel and `iterations` filter launches
#endif

}  // namespace art
