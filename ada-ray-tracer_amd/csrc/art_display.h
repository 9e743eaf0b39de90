// art_display.h -- the per-pixel text of art_auto_exposure_device and art_display_device (include/art_hip.h states the arithmetic; this
// is its one definition).  ART_HD functions over plain pointers, no HIP types: art_display.hip compiles them for gfx950 and
// tests/display_host compiles the same text with g++ (the arrangement of art_svgf_spatial.h with tests/svgf_spatial_host), so the
// kernels and the host build cannot drift apart.
//
// The transcendentals are ART-M1's (art_math.h: m1::log_pos, m1::exp_small through apow), the luminance is art_bind_moments'
// (colour_lum) and ART_CURVE_REFERENCE is resolve_pixel itself (art_shade.h), called, not retyped.
#pragma once
#include <stdint.h>
#include "art_hip.h"
#include "art_shade.h"

namespace art {
namespace dp {

constexpr int kBins = 256;                   // bin 0: pixels without a luminance; 1 .. 254: the range; 255: never written
constexpr int kStateWords = 4 + kBins;       // exposure, mean_log2, counted, frames, then the histogram

ART_HD bool finite_f(float v) { return (__builtin_bit_cast(uint32_t, v) & 0x7f800000u) != 0x7f800000u; }

struct ExposureParams {
  int32_t W, H;
  float scale, min_log2, max_log2, low_fraction, high_fraction, key, adapt, min_exposure, max_exposure;
};
struct DisplayParams {
  int32_t W, H;
  float scale, exposure, white;
  int32_t curve, transfer, dither, layout;
};

inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const char* x = (const char*)a; const char* y = (const char*)b;
  return a && b && x < y + nb && y < x + na;
}

// ArtExposureParams and the pointers -> the kernels' params: every refusal that needs no device.  Returns nullptr, or why the call is
// refused.  The library (art_device_entries.cpp) and tests/display_host both derive their params here.
inline const char* params_from_abi(const ArtExposureParams* p, const void* color3f, const void* state, ExposureParams& P) {
  if (!p) return "null ArtExposureParams";
  if (!color3f || !state) return "null color3f or state";
  if (p->width < 1 || p->height < 1 || (int64_t)p->width * p->height > (1ll << 28)) return "width and height must be at least 1 and width * height at most 2^28";
  if (!finite_f(p->scale)) return "scale is not finite";
  if (!(p->min_log2 >= -126.0f && p->max_log2 <= 127.0f && p->min_log2 < p->max_log2)) return "min_log2 and max_log2 must be finite, -126 <= min_log2 < max_log2 <= 127";
  if (!(p->low_fraction >= 0.0f && p->high_fraction <= 1.0f && p->low_fraction < p->high_fraction)) return "the fractions must be 0 <= low_fraction < high_fraction <= 1";
  if (!(finite_f(p->key) && p->key > 0.0f)) return "key must be finite and positive";
  if (!(finite_f(p->min_exposure) && finite_f(p->max_exposure) && p->min_exposure > 0.0f && p->min_exposure <= p->max_exposure)) return "the exposure bounds must be finite, 0 < min_exposure <= max_exposure";
  if (!(p->adapt > 0.0f && p->adapt <= 1.0f)) return "adapt must be in (0, 1]";
  if (((uintptr_t)state & 3) != 0) return "state is not 4-byte aligned";
  if (overlap(color3f, 12 * (size_t)p->width * (size_t)p->height, state, 4 * (size_t)kStateWords)) return "state overlaps color3f";
  P.W = p->width; P.H = p->height; P.scale = p->scale; P.min_log2 = p->min_log2; P.max_log2 = p->max_log2;
  P.low_fraction = p->low_fraction; P.high_fraction = p->high_fraction; P.key = p->key; P.adapt = p->adapt;
  P.min_exposure = p->min_exposure; P.max_exposure = p->max_exposure;
  return nullptr;
}

inline const char* params_from_abi(const ArtDisplayParams* p, const void* color3f, const void* exposure_state, const void* screen1u, const void* ldr3f, DisplayParams& P) {
  if (!p) return "null ArtDisplayParams";
  if (!color3f) return "null color3f";
  if (!screen1u && !ldr3f) return "screen1u and ldr3f are both null";
  if (p->width < 1 || p->height < 1 || (int64_t)p->width * p->height > (1ll << 28)) return "width and height must be at least 1 and width * height at most 2^28";
  if (!finite_f(p->scale)) return "scale is not finite";
  if (p->curve < ART_CURVE_REFERENCE || p->curve > ART_CURVE_ACES) return "unknown curve";
  if (p->transfer < ART_TRANSFER_SQRT || p->transfer > ART_TRANSFER_GAMMA22) return "unknown transfer";
  if (p->layout != ART_LAYOUT_ADA_XY && p->layout != ART_LAYOUT_ROW_MAJOR) return "unknown layout";
  if (p->dither != 0 && p->dither != 1) return "dither must be 0 or 1";
  if (!(finite_f(p->white) && p->white > 0.0f)) return "white must be finite and positive";
  if (!exposure_state && !(finite_f(p->exposure) && p->exposure >= 0.0f)) return "exposure must be finite and not negative";
  if (p->curve == ART_CURVE_REFERENCE && ldr3f) return "ldr3f is not defined for ART_CURVE_REFERENCE";
  const size_t N = (size_t)p->width * (size_t)p->height;
  if (overlap(color3f, 12 * N, screen1u, 4 * N)) return "screen1u overlaps color3f";
  if (overlap(color3f, 12 * N, ldr3f, 12 * N)) return "ldr3f overlaps color3f";
  if (overlap(screen1u, 4 * N, ldr3f, 12 * N)) return "ldr3f overlaps screen1u";
  if (overlap(exposure_state, 4 * (size_t)kStateWords, screen1u, 4 * N)) return "screen1u overlaps exposure_state";
  if (overlap(exposure_state, 4 * (size_t)kStateWords, ldr3f, 12 * N)) return "ldr3f overlaps exposure_state";
  P.W = p->width; P.H = p->height; P.scale = p->scale; P.exposure = p->exposure; P.white = p->white;
  P.curve = p->curve; P.transfer = p->transfer; P.dither = p->dither; P.layout = p->layout;
  return nullptr;
}

// ---- auto-exposure -----------------------------------------------------------------------------------------------------------------
// pixel p's histogram bin
ART_HD int exposure_bin(const ExposureParams& P, const float* color, size_t p) {
  const f3 c = mk3(color[3 * p] * P.scale, color[3 * p + 1] * P.scale, color[3 * p + 2] * P.scale);
  const float l = colour_lum(c);
  if (!finite_f(l) || !(l > 0.0f)) return 0;
  const double L = m1::log_pos((double)l) * 0x1.71547652b82fep+0;
  const double t = ((L - (double)P.min_log2) / ((double)P.max_log2 - (double)P.min_log2)) * 254.0;
  if (t < 0.0) return 1;
  if (t >= 253.0) return 254;
  return 1 + (int)t;                         // t >= 0: the conversion truncates, which is floor
}

// the walk over the finished histogram: state's four words from its 256 bins
ART_HD void exposure_from_histogram(const ExposureParams& P, uint32_t* state) {
  const uint32_t* hist = state + 4;
  const uint32_t frames = state[3];
  const float prev = __builtin_bit_cast(float, state[0]);
  uint64_t total = 0;
  for (int i = 1; i <= 254; ++i) total += hist[i];
  const double N = (double)total;
  const double a = (double)P.low_fraction * N, b = (double)P.high_fraction * N;
  const double lo2 = (double)P.min_log2, span = (double)P.max_log2 - (double)P.min_log2;
  double W = 0.0, S = 0.0, cum = 0.0;
  for (int i = 1; i <= 254; ++i) {
    const double lo = cum, hi = cum + (double)hist[i];
    const double o = (hi < b ? hi : b) - (lo > a ? lo : a);
    const double centre = lo2 + (((double)(i - 1) + 0.5) / 254.0) * span;
    if (o > 0.0) { W += o; S += o * centre; }
    cum = hi;
  }
  if (total == 0 || !(W > 0.0)) {
    state[0] = __builtin_bit_cast(uint32_t, frames ? prev : 1.0f);
    if (!frames) state[1] = 0u;
    state[2] = 0u;
    return;
  }
  const float m = (float)(S / W);
  const float target = aclamp(P.key * apow(2.0f, -m), P.min_exposure, P.max_exposure);
  const float e = frames ? prev + (target - prev) * P.adapt : target;
  state[0] = __builtin_bit_cast(uint32_t, e);
  state[1] = __builtin_bit_cast(uint32_t, m);
  state[2] = (uint32_t)total;
  state[3] = (frames == 0xffffffffu) ? frames : frames + 1u;
}

// ---- display -----------------------------------------------------------------------------------------------------------------------
ART_HD float display_channel(const DisplayParams& P, float c, float k) {
  float x = c * k;
  if (!finite_f(x) || !(x > 0.0f)) x = 0.0f;
  x = amin(x, 0x1p+60f);
  float v = x;
  if (P.curve == ART_CURVE_REINHARD) v = (x * (1.0f + x / (P.white * P.white))) / (1.0f + x);
  else if (P.curve == ART_CURVE_ACES) v = (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f);
  v = aclamp(v, 0.0f, 1.0f);
  if (P.transfer == ART_TRANSFER_SQRT) return sqrtf(v);
  if (P.transfer == ART_TRANSFER_SRGB) return (v < 0.0031308f) ? 12.92f * v : 1.055f * apow(v, 0x1.aaaaaap-2f) - 0.055f;
  return apow(v, 0x1.d1745ep-2f);
}

ART_HD uint32_t display_quantise(const DisplayParams& P, float u, int x, int y) {
  const float s = u * 255.0f;
  uint32_t q;
  if (P.dither) {
    // the 4 x 4 Bayer matrix {{0, 8, 2, 10}, {12, 4, 14, 6}, {3, 11, 1, 9}, {15, 7, 13, 5}}, four bits per entry, row y & 3 in bits 16 (y & 3) on
    const uint32_t B = (uint32_t)(0x5d7f91b36e4ca280ull >> (16 * (y & 3) + 4 * (x & 3))) & 15u;
    q = (uint32_t)(s + ((float)B + 0.5f) / 16.0f);
  } else q = ada_round_u32(s);
  return q < 255u ? q : 255u;
}

// where pixel (x, y)'s outputs go
ART_HD size_t display_index(const DisplayParams& P, int x, int y) {
  return P.layout == ART_LAYOUT_ADA_XY ? (size_t)x * (size_t)P.H + (size_t)y : (size_t)y * (size_t)P.W + (size_t)x;
}

// pixel (x, y) of the frame: its screen word and its three ldr floats (each plane may be null); e: the exposure
ART_HD void display_pixel(const DisplayParams& P, const float* color, float e, uint32_t* screen, float* ldr, int x, int y) {
  const size_t p = (size_t)y * (size_t)P.W + (size_t)x, o = display_index(P, x, y);
  const f3 c = mk3(color[3 * p], color[3 * p + 1], color[3 * p + 2]);
  if (P.curve == ART_CURVE_REFERENCE) {
    if (screen) screen[o] = resolve_pixel(c, P.scale);
    return;
  }
  const float k = P.scale * e;
  const float r = display_channel(P, c.x, k), g = display_channel(P, c.y, k), b = display_channel(P, c.z, k);
  if (ldr) { ldr[3 * o] = r; ldr[3 * o + 1] = g; ldr[3 * o + 2] = b; }
  if (screen) screen[o] = display_quantise(P, r, x, y) | (display_quantise(P, g, x, y) << 8) | (display_quantise(P, b, x, y) << 16);
}

}  // namespace dp

// ---- launch interface (art_display.hip); hipcc only: the g++ build of the tests takes the text above and nothing else
#if defined(__HIPCC__)
struct ExposureArgs { dp::ExposureParams P; int32_t n; const float* color; uint32_t* state; };
struct DisplayArgs { dp::DisplayParams P; const float* color; const uint32_t* state; uint32_t* screen; float* ldr; };
void launch_auto_exposure(hipStream_t st, const ExposureArgs& A);      // the histogram words are zeroed on st first
void launch_display(hipStream_t st, const DisplayArgs& A);
#endif

}  // namespace art
