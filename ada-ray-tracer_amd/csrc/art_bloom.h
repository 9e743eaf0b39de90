// art_bloom.h -- the per-texel text of art_bloom_device (include/art_hip.h states the arithmetic; this is its one definition): the read
// rule and the soft knee of a frame pixel, the 13-tap downsample of a texel (with the Karis boxes of the first one), the 2 x bilinear
// upsample, the blend on the way up, the mix, the sweep of the small levels that one workgroup does, and the refusals of the call's
// arguments.  ART_HD functions over plain pointers, no HIP types: art_bloom.hip compiles them for gfx950 and tests/bloom_host compiles
// the same text with g++ (the arrangement of art_firefly.h with tests/firefly_host), so the kernels and the host build cannot drift
// apart.  The luminance is dn::lum3 and the record dn::Rec4 (art_denoise.h), used, not retyped.
//
// Working data (the library's scratch): levels 1 .. M of the pyramid one after the other, level k at record off[k], row-major, one
// Rec4 {r, g, b, +0} per texel.  The down sweep writes D_k, the up sweep overwrites it with U_k: a texel's own D_k is all it reads of
// its level.  The filters take their texels through an accessor, so the same text runs over a tile staged in LDS (indices clamped
// while staging), over the levels of the tail in LDS, and over host arrays.
#pragma once
#include <stdint.h>
#include "art_hip.h"
#include "art_denoise.h"

namespace art {
namespace bl {

using dn::finite_f;
using dn::Rec4;

constexpr int kMaxLevels = 8;
// The tail's capacity: the records one workgroup holds in LDS.  64 KB per workgroup is the ceiling the call allows itself (a CU has
// 160 KB: a second workgroup of another kernel still fits beside it); 65536 / 16 = 4096 records hold a first level of up to 3072
// texels with everything below it (each level is a quarter of the one above, rounded up), e.g. 60 x 34 of a 1920 x 1080 frame.
constexpr int kTailTexels = 4096;
constexpr int kTailLanes = 1024;

struct T3 { float r, g, b; };
ART_HD T3 operator+(const T3& a, const T3& b) { return T3{a.r + b.r, a.g + b.g, a.b + b.b}; }
ART_HD T3 operator-(const T3& a, const T3& b) { return T3{a.r - b.r, a.g - b.g, a.b - b.b}; }
ART_HD T3 operator*(float k, const T3& a) { return T3{k * a.r, k * a.g, k * a.b}; }
ART_HD T3 operator*(const T3& a, float k) { return T3{a.r * k, a.g * k, a.b * k}; }
ART_HD T3 operator/(const T3& a, float k) { return T3{a.r / k, a.g / k, a.b / k}; }
ART_HD T3 texel(const Rec4& c) { return T3{c.x, c.y, c.z}; }
ART_HD Rec4 record(const T3& t) { return Rec4{t.r, t.g, t.b, 0.0f}; }
ART_HD int clampi(int i, int n) { return i < 0 ? 0 : i > n - 1 ? n - 1 : i; }

struct Params {
  int32_t W, H;
  int32_t made;                    // M: the levels made, 1 .. 8
  int32_t tail;                    // the first level of the tail (1 .. M - 1), or 0: every level has launches of its own
  int32_t karis, prefilter;        // prefilter: threshold or knee is not 0
  float scale, exposure, threshold, knee, scatter, strength;
  int32_t w[kMaxLevels + 1], h[kMaxLevels + 1];      // w[0] x h[0] is the frame
  uint32_t off[kMaxLevels + 2];    // level k's first record; off[M + 1]: the records in all (< 2^27 at 2^28 pixels)
};

// ---- read and prefilter ------------------------------------------------------------------------------------------------------------
ART_HD float read_channel(float scale, float c) {
  float s = scale * c;
  if (!finite_f(s) || !(s > 0.0f)) s = 0.0f;
  return amin(s, 0x1p+60f);
}
ART_HD T3 read_pixel(const Params& P, const float* color, size_t p) {
  return T3{read_channel(P.scale, color[3 * p]), read_channel(P.scale, color[3 * p + 1]), read_channel(P.scale, color[3 * p + 2])};
}
// the quadratic soft knee on e * luminance: the factor on s, in [0, 1]
ART_HD float knee_factor(const Params& P, float e, const T3& s) {
  const float l = e * dn::lum3(s.r, s.g, s.b);
  if (!finite_f(l) || !(l > 0.0f)) return 0.0f;
  const float q = aclamp(l - (P.threshold - P.knee), 0.0f, 2.0f * P.knee);
  const float soft = P.knee > 0.0f ? (q * q) / (4.0f * P.knee) : 0.0f;
  const float c = amax(soft, amax(l - P.threshold, 0.0f));
  return amin(c / l, 1.0f);
}
// L0(p): what the first downsample reads of frame pixel p.  e is asked for only when there is a prefilter.
template <class Exposure>
ART_HD T3 level0_pixel(const Params& P, const float* color, size_t p, Exposure exposure) {
  const T3 s = read_pixel(P, color, p);
  return P.prefilter ? knee_factor(P, exposure(), s) * s : s;
}

// ---- down --------------------------------------------------------------------------------------------------------------------------
// at(j, i): t[i][j], the texel of column 2 x - 2 + j and row 2 y - 2 + i of the level above, indices clamped
template <class At>
ART_HD T3 quad(At at, int a, int b) { return ((at(a, b) + at(a + 1, b)) + (at(a, b + 1) + at(a + 1, b + 1))) * 0.25f; }

template <bool KARIS, class At>
ART_HD T3 down13(At at) {
  const T3 q00 = quad(at, 0, 0), q20 = quad(at, 2, 0), q40 = quad(at, 4, 0), q11 = quad(at, 1, 1), q31 = quad(at, 3, 1);
  const T3 q02 = quad(at, 0, 2), q22 = quad(at, 2, 2), q42 = quad(at, 4, 2), q13 = quad(at, 1, 3), q33 = quad(at, 3, 3);
  const T3 q04 = quad(at, 0, 4), q24 = quad(at, 2, 4), q44 = quad(at, 4, 4);
  const T3 inner = (q11 + q31) + (q13 + q33);
  if constexpr (!KARIS) {
    const T3 edge = (q20 + q02) + (q42 + q24), corner = (q00 + q40) + (q04 + q44);
    return (0.125f * (inner + q22) + 0.0625f * edge) + 0.03125f * corner;
  } else {
    const T3 g0 = inner * 0.25f, g1 = ((q00 + q20) + (q02 + q22)) * 0.25f, g2 = ((q20 + q40) + (q22 + q42)) * 0.25f;
    const T3 g3 = ((q02 + q22) + (q04 + q24)) * 0.25f, g4 = ((q22 + q42) + (q24 + q44)) * 0.25f;
    const float k0 = 0.5f / (1.0f + dn::lum3(g0.r, g0.g, g0.b)), k1 = 0.125f / (1.0f + dn::lum3(g1.r, g1.g, g1.b));
    const float k2 = 0.125f / (1.0f + dn::lum3(g2.r, g2.g, g2.b)), k3 = 0.125f / (1.0f + dn::lum3(g3.r, g3.g, g3.b));
    const float k4 = 0.125f / (1.0f + dn::lum3(g4.r, g4.g, g4.b));
    const float K = ((k1 + k2) + (k3 + k4)) + k0;
    return ((((k1 * g1) + (k2 * g2)) + ((k3 * g3) + (k4 * g4))) + (k0 * g0)) / K;
  }
}

// ---- up, blend, mix ----------------------------------------------------------------------------------------------------------------
// at(dx, dy): the texel of the coarser level at (xn, yn) for 0 and at the far neighbour (one before for an even coordinate, one after
// for an odd one, clamped) for 1
template <class At>
ART_HD T3 up2(At at) {
  const T3 top = 0.75f * at(0, 0) + 0.25f * at(1, 0), bot = 0.75f * at(0, 1) + 0.25f * at(1, 1);
  return 0.75f * top + 0.25f * bot;
}
ART_HD int far_step(int v) { return (v & 1) ? 1 : -1; }
ART_HD T3 blend(const Params& P, const T3& d, const T3& up) { return d + P.scatter * (up - d); }
// pixel p of the frame: its words of the outputs (each may be null).  color and out may be the same plane: the pixel's own words are
// read before its first store.
ART_HD void mix_pixel(const Params& P, const float* color, size_t p, const T3& B, float* out, float* bloom) {
  if (out) {
    const T3 s = read_pixel(P, color, p);
    const T3 o = s + P.strength * (B - s);
    out[3 * p] = o.r; out[3 * p + 1] = o.g; out[3 * p + 2] = o.b;
  }
  if (bloom) { bloom[3 * p] = B.r; bloom[3 * p + 1] = B.g; bloom[3 * p + 2] = B.b; }
}

// ---- whole levels over a row-major array (the tail's LDS, host arrays) ---------------------------------------------------------------
// texel i of a level of wd columns from the level above, ws x hs at src
ART_HD T3 down_texel(const Rec4* src, int ws, int hs, int wd, int i) {
  const int y = i / wd, x = i - y * wd;
  return down13<false>([&](int j, int ii) { return texel(src[(size_t)clampi(2 * y - 2 + ii, hs) * (size_t)ws + (size_t)clampi(2 * x - 2 + j, ws)]); });
}
// up(S)(x, y) from the level S below, ws x hs at src
ART_HD T3 up_texel(const Rec4* src, int ws, int hs, int x, int y) {
  const int xn = x >> 1, yn = y >> 1, xf = clampi(xn + far_step(x), ws), yf = clampi(yn + far_step(y), hs);
  return up2([&](int dx, int dy) { return texel(src[(size_t)(dy ? yf : yn) * (size_t)ws + (size_t)(dx ? xf : xn)]); });
}

// The tail: levels P.tail .. M lie in L (level k at L + off[k] - off[P.tail]), D_tail filled in.  tail_down makes every level below it,
// tail_up turns every level from M - 1 back to the tail into U_k; `lanes` lanes share the texels, of which this is `lane`, and
// barrier() makes the lanes' stores visible to each other (nothing on the host, where one lane does it all).  No texel is written
// while another lane may read it: a down step writes level k + 1 and reads level k, an up step writes level k, of which a lane reads
// its own texel only, and reads level k + 1.
template <class Barrier>
ART_HD void tail_down(const Params& P, Rec4* L, int lane, int lanes, Barrier barrier) {
  const uint32_t o = P.off[P.tail];
  for (int k = P.tail; k < P.made; ++k) {
    barrier();
    const int n = P.w[k + 1] * P.h[k + 1];
    for (int i = lane; i < n; i += lanes) L[P.off[k + 1] - o + i] = record(down_texel(L + (P.off[k] - o), P.w[k], P.h[k], P.w[k + 1], i));
  }
}
template <class Barrier>
ART_HD void tail_up(const Params& P, Rec4* L, int lane, int lanes, Barrier barrier) {
  const uint32_t o = P.off[P.tail];
  for (int k = P.made - 1; k >= P.tail; --k) {
    barrier();
    const int n = P.w[k] * P.h[k];
    for (int i = lane; i < n; i += lanes) {
      const int y = i / P.w[k], x = i - y * P.w[k];
      Rec4* d = L + (P.off[k] - o) + i;
      *d = record(blend(P, texel(*d), up_texel(L + (P.off[k + 1] - o), P.w[k + 1], P.h[k + 1], x, y)));
    }
  }
  barrier();
}

// ---- the ABI's parameters and the pointers -> Params: every refusal that needs no device.  Returns nullptr, or why the call is refused.
// The library (art_device_entries.cpp) and tests/bloom_host both derive their Params here.
constexpr size_t kStateBytes = 1040;      // art_exposure_state_bytes()

inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const char* x = (const char*)a; const char* y = (const char*)b;
  return a && b && x < y + nb && y < x + na;
}

inline const char* params_from_abi(const ArtBloomParams* p, const void* color3f, const void* exposure_state, const void* out3f, const void* bloom3f, Params& P) {
  if (!p) return "null ArtBloomParams";
  if (!color3f) return "null color3f";
  if (!out3f && !bloom3f) return "out3f and bloom3f are both null";
  if (p->width < 1 || p->height < 1 || (int64_t)p->width * p->height > (1ll << 28)) return "width and height must be at least 1 and width * height at most 2^28";
  if (p->levels < 1 || p->levels > kMaxLevels) return "levels must be 1 .. 8";
  if (p->karis != 0 && p->karis != 1) return "karis must be 0 or 1";
  if (p->variant != 0 && p->variant != 1) return "variant must be 0 or 1";
  if (!finite_f(p->scale)) return "scale is not finite";
  if (!(finite_f(p->threshold) && p->threshold >= 0.0f)) return "threshold must be finite and not negative";
  if (!(finite_f(p->knee) && p->knee >= 0.0f)) return "knee must be finite and not negative";
  if (!(p->scatter >= 0.0f && p->scatter <= 1.0f)) return "scatter must be in [0, 1]";
  if (!(p->strength >= 0.0f && p->strength <= 1.0f)) return "strength must be in [0, 1]";
  if (!exposure_state && !(finite_f(p->exposure) && p->exposure >= 0.0f)) return "exposure must be finite and not negative";
  const size_t N = (size_t)p->width * (size_t)p->height;
  if (out3f != color3f && overlap(color3f, 12 * N, out3f, 12 * N)) return "out3f overlaps color3f (only out3f == color3f may share memory)";
  if (overlap(color3f, 12 * N, bloom3f, 12 * N)) return "bloom3f overlaps color3f";
  if (overlap(out3f, 12 * N, bloom3f, 12 * N)) return "bloom3f overlaps out3f";
  if (overlap(exposure_state, kStateBytes, out3f, 12 * N)) return "out3f overlaps exposure_state";
  if (overlap(exposure_state, kStateBytes, bloom3f, 12 * N)) return "bloom3f overlaps exposure_state";
  P.W = p->width; P.H = p->height; P.karis = p->karis;
  P.scale = p->scale; P.exposure = p->exposure; P.threshold = p->threshold; P.knee = p->knee; P.scatter = p->scatter; P.strength = p->strength;
  P.prefilter = (p->threshold != 0.0f || p->knee != 0.0f) ? 1 : 0;
  for (int k = 0; k <= kMaxLevels; ++k) { P.w[k] = P.h[k] = 0; P.off[k] = 0; }
  P.w[0] = P.W; P.h[0] = P.H; P.made = 0; P.off[1] = 0;
  for (int k = 1; k <= p->levels; ++k) {
    P.w[k] = (P.w[k - 1] + 1) >> 1; P.h[k] = (P.h[k - 1] + 1) >> 1;
    P.off[k + 1] = P.off[k] + (uint32_t)P.w[k] * (uint32_t)P.h[k];
    P.made = k;
    if (P.w[k] == 1 && P.h[k] == 1) break;
  }
  // variant 0: the tail starts at the first level that fits the workgroup's LDS together with everything below it, if a level follows it
  P.tail = 0;
  if (p->variant == 0)
    for (int k = 1; k < P.made; ++k)
      if (P.off[P.made + 1] - P.off[k] <= (uint32_t)kTailTexels) { P.tail = k; break; }
  return nullptr;
}

// The call over host arrays, texel after texel: what the kernels compute.  pyr: off[M + 1] records; down: null, or as many records
// that receive the pyramid as the down sweep left it; e: the exposure (the state's word 0 or p->exposure).
inline void run_host(const Params& P, const float* color, float e, Rec4* pyr, Rec4* down, float* out, float* bloom) {
  for (int i = 0; i < P.w[1] * P.h[1]; ++i) {
    const int y = i / P.w[1], x = i - y * P.w[1];
    auto at = [&](int j, int ii) {
      return level0_pixel(P, color, (size_t)clampi(2 * y - 2 + ii, P.H) * (size_t)P.W + (size_t)clampi(2 * x - 2 + j, P.W), [&] { return e; });
    };
    pyr[i] = record(P.karis ? down13<true>(at) : down13<false>(at));
  }
  const int last = P.tail ? P.tail : P.made;         // the levels with launches of their own end here
  for (int k = 1; k < last; ++k)
    for (int i = 0; i < P.w[k + 1] * P.h[k + 1]; ++i) pyr[P.off[k + 1] + i] = record(down_texel(pyr + P.off[k], P.w[k], P.h[k], P.w[k + 1], i));
  if (P.tail) {
    // one "lane" does the workgroup's sweep, in a buffer of the workgroup's capacity
    Rec4* L = new Rec4[kTailTexels];
    const uint32_t n = P.off[P.made + 1] - P.off[P.tail];
    for (int i = 0; i < P.w[P.tail] * P.h[P.tail]; ++i) L[i] = pyr[P.off[P.tail] + i];
    tail_down(P, L, 0, 1, [] {});
    if (down) for (uint32_t i = 0; i < n; ++i) down[P.off[P.tail] + i] = L[i];
    tail_up(P, L, 0, 1, [] {});
    if (down) for (uint32_t i = 0; i < P.off[P.tail]; ++i) down[i] = pyr[i];
    for (uint32_t i = 0; i < n; ++i) pyr[P.off[P.tail] + i] = L[i];
    delete[] L;
  } else if (down) {
    for (uint32_t i = 0; i < P.off[P.made + 1]; ++i) down[i] = pyr[i];
  }
  for (int k = last - 1; k >= 1; --k)
    for (int i = 0; i < P.w[k] * P.h[k]; ++i) {
      const int y = i / P.w[k], x = i - y * P.w[k];
      Rec4* d = pyr + P.off[k] + i;
      *d = record(blend(P, texel(*d), up_texel(pyr + P.off[k + 1], P.w[k + 1], P.h[k + 1], x, y)));
    }
  for (int y = 0; y < P.H; ++y)
    for (int x = 0; x < P.W; ++x) mix_pixel(P, color, (size_t)y * (size_t)P.W + (size_t)x, up_texel(pyr, P.w[1], P.h[1], x, y), out, bloom);
}

}  // namespace bl

// ---- launch interface (art_bloom.hip); hipcc only: the g++ build of the tests takes the text above and nothing else
#if defined(__HIPCC__)
struct BloomArgs {
  bl::Params P;
  const float* color; const uint32_t* state;      // state: nullptr = P.exposure
  float* out; float* bloom;                        // each may be nullptr
  bl::Rec4* pyr;                                   // the library's scratch, P.off[P.made + 1] records
};
void launch_bloom(hipStream_t st, const BloomArgs& A);      // every launch of the call, in order
#endif

}  // namespace art
