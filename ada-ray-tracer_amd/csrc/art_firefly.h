// art_firefly.h -- the per-pixel text of art_firefly_device (include/art_hip.h states the arithmetic; this is its one definition): the key
// of a pixel, the rank-th largest key of a window, the limit and the result of a pixel, and the refusals of the call's arguments.  ART_HD
// functions over plain pointers, no HIP types: art_firefly.hip compiles them for gfx950 and tests/firefly_host compiles the same text with
// g++ (the arrangement of art_svgf_spatial.h with tests/svgf_spatial_host), so the kernels and the host build cannot drift apart.  The
// luminance is dn::lum3 (art_denoise.h), called, not retyped.
//
// Working data (the library's scratch): one key per pixel, row-major -- l(q), or the quiet NaN for a bad pixel.  The window reads keys
// only, never the colour, which is what lets out3f be color3f.  A position outside the frame reads as the quiet NaN as well: "not a
// neighbour" is one test, key != key.
#pragma once
#include <stdint.h>
#include "art_hip.h"
#include "art_denoise.h"

namespace art {
namespace fi {

using dn::finite_f;

struct Params {
  int32_t W, H;
  int32_t radius, rank, min_count;
  float scale, gain, floor;       // floor: the ABI's + 0.0f
};

ART_HD float qnan() { return __builtin_bit_cast(float, 0x7fc00000u); }
ART_HD float quiet(float v) { return (v != v) ? qnan() : v; }      // a NaN leaves as THE quiet NaN (art_adaptive.h)

// c(q) = scale * colour and the key of pixel q (a linear index)
ART_HD float key_of(const Params& P, const float* color, size_t q, float& r, float& g, float& b) {
  r = P.scale * color[3 * q]; g = P.scale * color[3 * q + 1]; b = P.scale * color[3 * q + 2];
  const float l = dn::lum3(r, g, b);
  return (finite_f(r) && finite_f(g) && finite_f(b) && finite_f(l)) ? l : qnan();
}

// The four largest keys seen, t0 >= t1 >= t2 >= t3, and how many keys were seen: four named floats, no indexed array.
struct Top4 { float t0, t1, t2, t3; int32_t count; };

ART_HD Top4 top4_empty() {
  const float ninf = __builtin_bit_cast(float, 0xff800000u);
  return Top4{ninf, ninf, ninf, ninf, 0};
}
// one step of the insertion: the larger of (t, a) stays in t, the smaller travels on in a
ART_HD void exchange(float& t, float& a) {
  const bool up = a > t;
  const float hi = up ? a : t, lo = up ? t : a;
  t = hi; a = lo;
}
// a key that is a NaN (a bad pixel, a position outside the frame, another id) is no neighbour
ART_HD void insert(Top4& t, float key) {
  const bool is = key == key;
  float a = is ? key : t.t3;      // (t3 against itself: nothing moves)
  t.count += is ? 1 : 0;
  exchange(t.t0, a); exchange(t.t1, a); exchange(t.t2, a); exchange(t.t3, a);
}
ART_HD float rank_of(const Top4& t, int rank) { return rank == 1 ? t.t0 : rank == 2 ? t.t1 : rank == 3 ? t.t2 : t.t3; }

// The window of a pixel whose id is idp: key_at(dx, dy) is the key at that offset (the quiet NaN outside the frame), id_at(dx, dy) the
// id there, asked only where the key is a number.  R: the radius; IDS: an id plane is given.
template <int R, bool IDS, class KeyAt, class IdAt>
ART_HD Top4 window(int32_t idp, KeyAt key_at, IdAt id_at) {
  Top4 t = top4_empty();
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int dy = -R; dy <= R; ++dy) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int dx = -R; dx <= R; ++dx) {
      if (dx == 0 && dy == 0) continue;
      float k = key_at(dx, dy);
      if constexpr (IDS) { if (k == k && id_at(dx, dy) != idp) k = qnan(); }
      insert(t, k);
    }
  }
  return t;
}

ART_HD float limit(const Params& P, float m) { return amax(P.gain * m + P.floor, 0.0f); }

// pixel p (a linear index) whose own key is kp and whose window gave t: its words of the outputs.  color and out, moments and moments_out
// may be the same planes: the pixel's inputs are all read before its first store.
ART_HD void resolve(const Params& P, const Top4& t, const float* color, const float* moments, size_t p, float* out, float* moments_out, uint8_t* clamped) {
  float r, g, b;
  const float l = key_of(P, color, p, r, g, b);
  float s1 = 0.0f, s2 = 0.0f;
  if (moments) { s1 = moments[2 * p]; s2 = moments[2 * p + 1]; }
  uint8_t flag = (l != l) ? 2 : 0;
  if (flag == 0 && t.count >= P.min_count) {
    const float T = limit(P, rank_of(t, P.rank));
    if (l > T) {
      const float f = T / l;
      r = f * r; g = f * g; b = f * b;
      s1 = quiet(f * s1); s2 = quiet((f * f) * s2);
      flag = 1;
    }
  }
  out[3 * p] = quiet(r); out[3 * p + 1] = quiet(g); out[3 * p + 2] = quiet(b);
  if (moments) { moments_out[2 * p] = s1; moments_out[2 * p + 1] = s2; }
  if (clamped) clamped[p] = flag;
}

// ---- the ABI's parameters and the pointers -> Params: every refusal that needs no device.  Returns nullptr, or why the call is refused.
// The library (art_device_entries.cpp) and tests/firefly_host both derive their Params here.
inline const char* params_from_abi(const ArtFireflyParams* p, const void* color3f, const void* moments2f, const void* out3f, const void* moments_out2f, Params& P) {
  if (!p) return "null ArtFireflyParams";
  if (!color3f || !out3f) return "null color3f or out3f";
  if (moments_out2f && !moments2f) return "moments_out2f is given without moments2f";
  if (moments2f && !moments_out2f) return "moments2f is given without moments_out2f";
  if (p->width < 1 || p->height < 1 || (int64_t)p->width * p->height > (1ll << 28)) return "width and height must be at least 1 and width * height at most 2^28";
  if (p->radius != 1 && p->radius != 2) return "radius must be 1 or 2";
  if (p->rank < 1 || p->rank > 4) return "rank must be 1 .. 4";
  if (p->min_count < p->rank || p->min_count > (2 * p->radius + 1) * (2 * p->radius + 1) - 1) return "min_count must be rank .. (2 * radius + 1)^2 - 1";
  if (!finite_f(p->scale)) return "scale is not finite";
  if (!finite_f(p->gain) || !(p->gain >= 1.0f)) return "gain must be finite and at least 1";
  if (!finite_f(p->floor) || !(p->floor >= 0.0f)) return "floor must be finite and at least 0";
  P.W = p->width; P.H = p->height; P.radius = p->radius; P.rank = p->rank; P.min_count = p->min_count;
  P.scale = p->scale; P.gain = p->gain; P.floor = p->floor + 0.0f;
  return nullptr;
}

// An output over another plane: lanes store while others still read.  out3f == color3f and moments_out2f == moments2f, the same
// address, are the two in-place uses the call allows.  (After the planes' own check.)
inline const char* overlap_refusal(const Params& P, const void* color3f, const void* moments2f, const void* id, const void* out3f, const void* moments_out2f,
                                   const void* clamped1b) {
  const size_t N = (size_t)P.W * (size_t)P.H;
  const struct { const void* p; size_t bytes; bool output; } pl[] = {{color3f, 12 * N, false}, {moments2f, 8 * N, false}, {id, 4 * N, false},
                                                                    {out3f, 12 * N, true}, {moments_out2f, 8 * N, true}, {clamped1b, N, true}};
  for (int a = 0; a < 6; ++a)
    for (int b = a + 1; b < 6; ++b) {
      if (!pl[a].p || !pl[b].p || !(pl[a].output || pl[b].output)) continue;
      if (pl[a].p == pl[b].p && ((a == 0 && b == 3) || (a == 1 && b == 4))) continue;
      const char* x = (const char*)pl[a].p; const char* y = (const char*)pl[b].p;
      if (x < y + pl[b].bytes && y < x + pl[a].bytes)
        return pl[a].output ? "two outputs overlap" : "an output overlaps an input plane (only out3f == color3f and moments_out2f == moments2f may share memory)";
    }
  return nullptr;
}

// The call over host arrays, pixel after pixel: what the two kernels compute.  keys: W * H floats of working memory.
template <int R, bool IDS>
inline void run_host(const Params& P, const float* color, const float* moments, const int32_t* id, float* keys, float* out, float* moments_out, uint8_t* clamped) {
  const size_t N = (size_t)P.W * (size_t)P.H;
  for (size_t q = 0; q < N; ++q) { float r, g, b; keys[q] = key_of(P, color, q, r, g, b); }
  for (int y = 0; y < P.H; ++y)
    for (int x = 0; x < P.W; ++x) {
      const size_t p = (size_t)y * (size_t)P.W + (size_t)x;
      auto inside = [&](int dx, int dy) { return x + dx >= 0 && x + dx < P.W && y + dy >= 0 && y + dy < P.H; };
      auto at = [&](int dx, int dy) { return (size_t)(y + dy) * (size_t)P.W + (size_t)(x + dx); };
      const Top4 t = window<R, IDS>(IDS ? id[p] : 0, [&](int dx, int dy) { return inside(dx, dy) ? keys[at(dx, dy)] : qnan(); },
                                    [&](int dx, int dy) { return id[at(dx, dy)]; });
      resolve(P, t, color, moments, p, out, moments_out, clamped);
    }
}

}  // namespace fi

// ---- launch interface (art_firefly.hip); hipcc only: the g++ build of the tests takes the text above and nothing else
#if defined(__HIPCC__)
// the caller's planes (nullptr: not given) and the library's key plane, W * H floats
struct FireflyArgs {
  fi::Params P;
  const float* color; const float* moments; const int32_t* id;
  float* out; float* moments_out; uint8_t* clamped;
  float* keys;
};
void launch_firefly(hipStream_t st, const FireflyArgs& A);      // the key kernel, then the window kernel over 16 x 16 tiles
#endif

}  // namespace art
