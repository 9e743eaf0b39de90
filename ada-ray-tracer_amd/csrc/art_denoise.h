// art_denoise.h -- the per-pixel text of art_denoise_device (include/art_hip.h states the arithmetic; this is its one definition).
// ART_HD functions over plain pointers, no HIP types: art_denoise.hip compiles them for gfx950 and tests/denoise_host compiles the same
// text with g++ (the arrangement of art_shade.h with tests/host_sim), so the kernel and the host build cannot drift apart.
//
// Working data (the library's scratch, one entry per pixel, row-major):
//   image   Rec4 {r, g, b, z}         c_i and the pixel's depth (0 without a depth plane); two of them, read and written in turn
//   guide   Rec4 {nx, ny, nz, flags}  the normal ((0, 0, 0) without a normal plane) and, as a word, bit 0 = bad in guides; constant over the iterations
//   grad    Rec2 {gx, gy}             the depth gradient, read for the centre only
// so a tap costs two 16-byte loads.  "Bad in colour" follows c_i (a repaired pixel is good in the next iteration) and is read off the
// tap's own colour.
#pragma once
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
    const int x1 = (x + 1 < P.W) ? x + 1 : P.W - 1, x0 = (x > 0) ? x - 1 : 0;
    const int y1 = (y + 1 < P.H) ? y + 1 : P.H - 1, y0 = (y > 0) ? y - 1 : 0;
    const size_t row = (size_t)y * (size_t)P.W;
    d.x = 0.5f * (depth[row + (size_t)x1] - depth[row + (size_t)x0]);
    d.y = 0.5f * (depth[(size_t)y1 * (size_t)P.W + (size_t)x] - depth[(size_t)y0 * (size_t)P.W + (size_t)x]);
  }
  g.w = __builtin_bit_cast(float, flags);
}

// iteration i at centre (x, y): c_{i+1} (with the centre's depth carried along in .w)
ART_HD Rec4 atrous_pixel(const Params& P, const Rec4* image, const Rec4* guide, const Rec2* grad, int x, int y, int i) {
  const int s = 1 << i;
  const size_t p = (size_t)y * (size_t)P.W + (size_t)x;
  const Rec4 cp = image[p], gp = guide[p];
  const Rec2 dp = grad[p];
  const bool centre_bad_colour = !finite_rgb(cp);
  const bool use_depth = P.has_depth && P.sigma_depth > 0.0f;
  const bool use_colour = P.sigma_color > 0.0f && !centre_bad_colour;
  const float lp = lum(cp);
  const float sc = P.sigma_color * __builtin_bit_cast(float, (uint32_t)(127 - i) << 23);      // sigma_color * 2^-i
  const float zfloor = 1e-3f * cp.w + 1e-6f;
  const f3 np = mk3(gp.x, gp.y, gp.z);
  float ar = 0.0f, ag = 0.0f, ab = 0.0f, wsum = 0.0f;
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
      const float h = spline(dx) * spline(dy);
      float w = h;
      if (dx != 0 || dy != 0) {
        float wn = 1.0f;
        if (P.has_normal) {
          wn = amax(dot(np, mk3(gq.x, gq.y, gq.z)), 0.0f);
          for (int j = 0; j < P.normal_log2; ++j) wn = wn * wn;
        }
        float xz = 0.0f;
        if (use_depth) xz = fabsf(cp.w - cq.w) / (P.sigma_depth * (fabsf(dp.x * (float)(s * dx)) + fabsf(dp.y * (float)(s * dy))) + zfloor);
        float xc = 0.0f;
        if (use_colour) xc = fabsf(lp - lum(cq)) / sc;
        const double t = -((double)xz + (double)xc);
        float e;
        if (t < -200.0) e = 0.0f;
        else if (t <= 0.0) e = (float)m1::exp_small(t);
        else e = __builtin_bit_cast(float, 0x7fc00000u);        // t NaN (or positive: a negative depth): the tap is skipped below
        w = (h * wn) * e;
        if (w != w) continue;
      }
      ar += w * cq.x; ag += w * cq.y; ab += w * cq.z;
      wsum += w;
    }
  }
  Rec4 r = cp;
  if (wsum > 0.0f) { r.x = ar / wsum; r.y = ag / wsum; r.z = ab / wsum; }
  return r;
}

// after the last iteration: the output of pixel p
ART_HD void finish_pixel(const Params& P, const float* albedo, size_t p, const Rec4& c, float& r, float& g, float& b) {
  r = c.x; g = c.y; b = c.z;
  if (P.demod) { r = r * albedo_floor(albedo[3 * p]); g = g * albedo_floor(albedo[3 * p + 1]); b = b * albedo_floor(albedo[3 * p + 2]); }
}

// ---- art_denoise_svgf_device: the variance-guided variant (include/art_hip.h states its arithmetic; the functions above are not touched) ----
// Working data, one entry per pixel, row-major:
//   image   Rec4 {r, g, b, v}         c_i and v_i, the variance of the pixel's luminance estimate; two of them, read and written in turn
//   guide   Rec4 {nx, ny, nz, flags}  as above, plus bit 1 = no colour stop when this pixel is the centre (its v was not finite)
//   z       float                     the depth, a plane of its own: read for a tap only when the depth stop is on
//   grad    Rec2 {gx, gy}             as above
// so a tap costs two 16-byte loads and, with a depth plane, one dword load; the variance prefilter reads the same two records of the
// centre's 3 x 3 neighbours.
constexpr uint32_t kNoColourStop = 2u;

ART_HD float lum3(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// preparation of pixel (x, y): pack_pixel's c_0, guide record and gradient, the depth on its own, and v_0 from the moments in binary64
ART_HD void svgf_pack_pixel(const Params& P, int32_t n_colours, const float* color, const float* moments, const float* albedo, const float* normal,
                            const float* depth, int x, int y, Rec4& c, Rec4& g, float& z, Rec2& d) {
  pack_pixel(P, color, albedo, normal, depth, x, y, c, g, d);
  z = c.w;
  const size_t p = (size_t)y * (size_t)P.W + (size_t)x;
  const double n = (double)n_colours;
  const double s1 = (double)moments[2 * p], s2 = (double)moments[2 * p + 1];
  const double D = s2 - (s1 * s1) / n;
  double v = (((D < 0.0) ? 0.0 : D) * (n / (n - 1.0))) * ((double)P.scale * (double)P.scale);
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

// art_denoise_svgf_var_device: the same preparation with v_0 from a variance plane (one float per pixel) instead of the moments
ART_HD void svgf_var_pack_pixel(const Params& P, const float* color, const float* variance, const float* albedo, const float* normal,
                                const float* depth, int x, int y, Rec4& c, Rec4& g, float& z, Rec2& d) {
  pack_pixel(P, color, albedo, normal, depth, x, y, c, g, d);
  z = c.w;
  const size_t p = (size_t)y * (size_t)P.W + (size_t)x;
  double v = (double)variance[p] * ((double)P.scale * (double)P.scale);
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

// iteration i at centre (x, y): {c_{i+1}, v_{i+1}}
ART_HD Rec4 svgf_atrous_pixel(const Params& P, const Rec4* image, const Rec4* guide, const float* zplane, const Rec2* grad, int x, int y, int i) {
  const int s = 1 << i;
  const size_t p = (size_t)y * (size_t)P.W + (size_t)x;
  const Rec4 cp = image[p], gp = guide[p];
  const Rec2 dp = grad[p];
  const bool use_depth = P.has_depth && P.sigma_depth > 0.0f;
  const float zp = P.has_depth ? zplane[p] : 0.0f;
  const bool use_colour = P.sigma_color > 0.0f && finite_rgb(cp) && !(__builtin_bit_cast(uint32_t, gp.w) & kNoColourStop);
  // the variance prefilter: 3 x 3 at spacing 1 over the taps that are inside, good in guides and finite in colour
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
  const float vg = (ks > 0.0f) ? vs / ks : 0.0f;
  const float lp = lum(cp);
  const float sc = P.sigma_color * sqrtf(vg) + 1e-6f;
  const float zfloor = 1e-3f * zp + 1e-6f;
  const f3 np = mk3(gp.x, gp.y, gp.z);
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
      const float h = spline(dx) * spline(dy);
      float w = h;
      if (dx != 0 || dy != 0) {
        float wn = 1.0f;
        if (P.has_normal) {
          wn = amax(dot(np, mk3(gq.x, gq.y, gq.z)), 0.0f);
          for (int j = 0; j < P.normal_log2; ++j) wn = wn * wn;
        }
        float xz = 0.0f;
        if (use_depth) xz = fabsf(zp - zplane[q]) / (P.sigma_depth * (fabsf(dp.x * (float)(s * dx)) + fabsf(dp.y * (float)(s * dy))) + zfloor);
        float xc = 0.0f;
        if (use_colour) xc = fabsf(lp - lum(cq)) / sc;
        const double t = -((double)xz + (double)xc);
        float e;
        if (t < -200.0) e = 0.0f;
        else if (t <= 0.0) e = (float)m1::exp_small(t);
        else e = __builtin_bit_cast(float, 0x7fc00000u);        // t NaN or positive: the tap is skipped below
        w = (h * wn) * e;
        if (w != w) continue;
      }
      ar += w * cq.x; ag += w * cq.y; ab += w * cq.z;
      av += (w * w) * cq.w;
      wsum += w;
    }
  }
  Rec4 r = cp;
  if (wsum > 0.0f) { r.x = ar / wsum; r.y = ag / wsum; r.z = ab / wsum; r.w = av / (wsum * wsum); }
  return r;
}

}  // namespace dn
}  // namespace art
