// art_upsample.h -- the per-pixel text of art_upsample_device (include/art_hip.h states the arithmetic; this is its one definition): the
// preparation of a lo pixel, the mapping and the taps of a hi pixel, and the refusals of the call's arguments.  ART_HD functions over
// plain pointers, no HIP types: art_upsample.hip compiles them for gfx950 and tests/upsample_host compiles the same text with g++ (the
// arrangement of art_denoise.h with tests/denoise_host), so the kernels and the host build cannot drift apart.  The edge-stopping weight
// is dn::stop_weight and the gradient dn::central_difference (art_denoise.h), called, not retyped.
//
// Working data (the library's scratch, one entry per LO pixel, row-major):
//   colour  Rec4 {r, g, b, z}         c(q) and the lo depth (0 without a depth plane)
//   guide   Rec4 {nx, ny, nz, word}   the lo normal ((0, 0, 0) without a normal plane) and, as a word, bit 0 = bad in guides, bit 1 = bad in colour
// so a tap costs two 16-byte loads; the lo id stays in the caller's plane (one dword more per tap where ids are given).
#pragma once
#include "art_denoise.h"

namespace art {
namespace us {

using dn::Rec4;

struct Params {
  int32_t W, H, LW, LH;
  int32_t footprint, demod, normal_log2;
  int32_t has_normal, has_depth, has_id;
  float scale, sigma_depth, jx, jy;
};

constexpr uint32_t kBadGuides = 1u, kBadColour = 2u;

ART_HD bool is_zero(const f3& n) { return n.x == 0.0f && n.y == 0.0f && n.z == 0.0f; }

// preparation of lo pixel q (a linear index): c(q) with the depth, the normal with the flags
ART_HD void pack_lo(const Params& P, const float* color, const float* albedo, const float* normal, const float* depth, size_t q, Rec4& c, Rec4& g) {
  c.x = P.scale * color[3 * q]; c.y = P.scale * color[3 * q + 1]; c.z = P.scale * color[3 * q + 2]; c.w = 0.0f;
  if (P.demod) {
    c.x = c.x / dn::albedo_floor(albedo[3 * q]); c.y = c.y / dn::albedo_floor(albedo[3 * q + 1]); c.z = c.z / dn::albedo_floor(albedo[3 * q + 2]);
  }
  uint32_t flags = dn::finite_rgb(c) ? 0u : kBadColour;
  g.x = g.y = g.z = 0.0f;
  if (P.has_normal) {
    g.x = normal[3 * q]; g.y = normal[3 * q + 1]; g.z = normal[3 * q + 2];
    if (!(dn::finite_f(g.x) && dn::finite_f(g.y) && dn::finite_f(g.z))) flags |= kBadGuides;
  }
  if (P.has_depth) {
    c.w = depth[q];
    if (!dn::finite_f(c.w)) flags |= kBadGuides;
  }
  g.w = __builtin_bit_cast(float, flags);
}

// one axis of the mapping: hi coordinate k of n to the lo frame of ln pixels: the first tap's base index, the fraction and the ratio
ART_HD void map_axis(int k, int n, int ln, float jitter, int& i0, float& f, float& s) {
  s = (float)ln / (float)n;
  const float u = ((float)k + 0.5f) * s - (0.5f + jitter);
  const float fl = floorf(u);
  i0 = (int)fl;
  f = u - fl;
}

template <int FOOT>
ART_HD float tap_weight(int a, float f) {
  if constexpr (FOOT == 2) return a == 0 ? 1.0f - f : f;
  else return amax(0.0f, 1.0f - fabsf((float)a - f) / 2.0f);
}

ART_HD int clamp_index(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

// The hi guides of one call (nullptr: not given) and the outputs of one pixel.
struct HiGuides { const float* albedo; const float* normal; const float* depth; const int32_t* id; };

// hi pixel (x, y): its colour and its fallback byte.  FOOT: the footprint; IDS: both id planes are given (lo_id is read only then)
template <int FOOT, bool IDS>
ART_HD void upsample_pixel(const Params& P, const Rec4* lo_c, const Rec4* lo_g, const int32_t* lo_id, const HiGuides& hi, int x, int y,
                           float& r, float& g, float& b, uint8_t& fallback) {
  constexpr int A0 = (FOOT == 2) ? 0 : -1, A1 = (FOOT == 2) ? 1 : 2;
  const size_t p = (size_t)y * (size_t)P.W + (size_t)x;
  int i0, j0; float fx, fy, sx, sy;
  map_axis(x, P.W, P.LW, P.jx, i0, fx, sx);
  map_axis(y, P.H, P.LH, P.jy, j0, fy, sy);
  f3 np = mk3(0.0f, 0.0f, 0.0f);
  float zp = 0.0f, gx = 0.0f, gy = 0.0f;
  bool bad = false;
  if (P.has_normal) {
    np = mk3(hi.normal[3 * p], hi.normal[3 * p + 1], hi.normal[3 * p + 2]);
    bad = !(dn::finite_f(np.x) && dn::finite_f(np.y) && dn::finite_f(np.z));
  }
  if (P.has_depth) {
    const float* depth = hi.depth;
    zp = depth[p];
    bad = bad || !dn::finite_f(zp);
    dn::central_difference(P.W, P.H, x, y, [depth](size_t k) { return depth[k]; }, gx, gy);
  }
  const bool background = P.has_normal && !bad && is_zero(np);
  int32_t idp = 0;
  if constexpr (IDS) idp = hi.id[p];
  const dn::Stops stops = {np, P.has_normal, P.normal_log2, P.has_depth && P.sigma_depth > 0.0f, zp, gx, gy, 1e-3f * zp + 1e-6f, P.sigma_depth};
  float ar = 0.0f, ag = 0.0f, ab = 0.0f, wsum = 0.0f;
  if (!bad) {
    for (int bb = A0; bb <= A1; ++bb) {
      const size_t row = (size_t)clamp_index(j0 + bb, P.LH) * (size_t)P.LW;
      const float ky = tap_weight<FOOT>(bb, fy), oy = ((float)bb - fy) / sy;
      for (int a = A0; a <= A1; ++a) {
        const size_t q = row + (size_t)clamp_index(i0 + a, P.LW);
        const Rec4 gq = lo_g[q];
        if (__builtin_bit_cast(uint32_t, gq.w) & (kBadGuides | kBadColour)) continue;
        if constexpr (IDS) { if (lo_id[q] != idp) continue; }
        const Rec4 cq = lo_c[q];
        const f3 nq = mk3(gq.x, gq.y, gq.z);
        float w = ky * tap_weight<FOOT>(a, fx);
        if (background) {
          if (!is_zero(nq)) continue;
        } else if (!dn::stop_weight(stops, w, nq, cq.w, ((float)a - fx) / sx, oy, 0.0f, w)) continue;
        ar += w * cq.x; ag += w * cq.y; ab += w * cq.z;
        wsum += w;
      }
    }
  }
  fallback = 0;
  if (!(wsum > 0.0f)) {                  // unguided: the same taps with w = h, all that are good in colour
    ar = ag = ab = wsum = 0.0f;
    for (int bb = A0; bb <= A1; ++bb) {
      const size_t row = (size_t)clamp_index(j0 + bb, P.LH) * (size_t)P.LW;
      const float ky = tap_weight<FOOT>(bb, fy);
      for (int a = A0; a <= A1; ++a) {
        const size_t q = row + (size_t)clamp_index(i0 + a, P.LW);
        if (__builtin_bit_cast(uint32_t, lo_g[q].w) & kBadColour) continue;
        const Rec4 cq = lo_c[q];
        const float w = ky * tap_weight<FOOT>(a, fx);
        ar += w * cq.x; ag += w * cq.y; ab += w * cq.z;
        wsum += w;
      }
    }
    fallback = 1;
  }
  if (wsum > 0.0f) { r = ar / wsum; g = ag / wsum; b = ab / wsum; }
  else { r = g = b = 0.0f; fallback = 2; }
  if (P.demod) {
    r = r * dn::albedo_floor(hi.albedo[3 * p]); g = g * dn::albedo_floor(hi.albedo[3 * p + 1]); b = b * dn::albedo_floor(hi.albedo[3 * p + 2]);
  }
}

// ---- the ABI's parameters and the pointers -> Params: every refusal that needs no device.  Returns nullptr, or why the call is refused.
// The library (art_device_entries.cpp) and tests/upsample_host both derive their Params here.
inline const char* params_from_abi(const ArtUpsampleParams* p, const void* lo_color3f, const ArtUpsampleGuides* lo, const ArtUpsampleGuides* hi, const void* out3f, Params& P) {
  if (!p) return "null ArtUpsampleParams";
  if (!lo_color3f || !out3f) return "null lo_color3f or out3f";
  if (!lo || !hi) return "null ArtUpsampleGuides (lo or hi)";
  if (p->width < 1 || p->height < 1 || (int64_t)p->width * p->height > (1ll << 28)) return "width and height must be at least 1 and width * height at most 2^28";
  if (p->lo_width < 1 || p->lo_width > p->width || p->lo_height < 1 || p->lo_height > p->height) return "lo_width must be 1 .. width and lo_height 1 .. height";
  if (p->footprint != 2 && p->footprint != 4) return "footprint must be 2 or 4";
  if (p->normal_log2 < 0 || p->normal_log2 > 10) return "normal_log2 must be 0 .. 10";
  if (!dn::finite_f(p->scale)) return "scale is not finite";
  if (p->sigma_depth != p->sigma_depth) return "sigma_depth is NaN";
  for (int k = 0; k < 2; ++k)
    if (!(p->jitter[k] > -0.5f && p->jitter[k] < 0.5f)) return "each jitter must be inside (-0.5, 0.5)";
  if ((lo->albedo3f != nullptr) != (hi->albedo3f != nullptr)) return "albedo3f is given on one side only";
  if ((lo->normal3f != nullptr) != (hi->normal3f != nullptr)) return "normal3f is given on one side only";
  if ((lo->depth != nullptr) != (hi->depth != nullptr)) return "depth is given on one side only";
  if ((lo->id != nullptr) != (hi->id != nullptr)) return "id is given on one side only";
  if (p->demodulate != 0 && !lo->albedo3f) return "demodulate needs the albedo planes";
  P.W = p->width; P.H = p->height; P.LW = p->lo_width; P.LH = p->lo_height;
  P.footprint = p->footprint; P.demod = p->demodulate != 0 ? 1 : 0; P.normal_log2 = p->normal_log2;
  P.has_normal = lo->normal3f ? 1 : 0; P.has_depth = lo->depth ? 1 : 0; P.has_id = lo->id ? 1 : 0;
  P.scale = p->scale; P.sigma_depth = p->sigma_depth; P.jx = p->jitter[0]; P.jy = p->jitter[1];
  return nullptr;
}

// An output over an input plane, or over the other output: lanes store while others still read.  (After the planes' own check.)
inline const char* overlap_refusal(const Params& P, const void* lo_color3f, const ArtUpsampleGuides* lo, const ArtUpsampleGuides* hi, const void* out3f, const void* fallback1b) {
  const size_t N = (size_t)P.W * (size_t)P.H, NL = (size_t)P.LW * (size_t)P.LH;
  const struct { const void* p; size_t bytes; } in[] = {{lo_color3f, 12 * NL}, {lo->albedo3f, 12 * NL}, {lo->normal3f, 12 * NL}, {lo->depth, 4 * NL}, {lo->id, 4 * NL},
                                                        {hi->albedo3f, 12 * N}, {hi->normal3f, 12 * N}, {hi->depth, 4 * N}, {hi->id, 4 * N}};
  auto overlap = [](const void* a, size_t na, const void* b, size_t nb) {
    const char* x = (const char*)a; const char* y = (const char*)b;
    return a && b && x < y + nb && y < x + na;
  };
  for (const auto& i : in) {
    if (overlap(i.p, i.bytes, out3f, 12 * N)) return "out3f overlaps an input plane";
    if (overlap(i.p, i.bytes, fallback1b, N)) return "fallback1b overlaps an input plane";
  }
  if (overlap(out3f, 12 * N, fallback1b, N)) return "fallback1b overlaps out3f";
  return nullptr;
}

}  // namespace us

// ---- launch interface (art_upsample.hip); hipcc only: the g++ build of the tests takes the text above and nothing else
#if defined(__HIPCC__)
// the caller's planes (nullptr: not given) and the library's scratch records, LW * LH of each
struct UpsampleArgs {
  us::Params P;
  const float* lo_color; const float* lo_albedo; const float* lo_normal; const float* lo_depth; const int32_t* lo_id;
  us::HiGuides hi;
  float* out; uint8_t* fallback;
  us::Rec4* lo_c; us::Rec4* lo_g;
};
void launch_upsample(hipStream_t st, const UpsampleArgs& A);      // the pack kernel over the lo frame, then the upsample kernel over the hi frame
#endif

}  // namespace art
