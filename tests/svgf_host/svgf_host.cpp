// TEST-ONLY: art_denoise_svgf_device and the accumulate with moments on host arrays, through the product's own per-pixel text
// (csrc/art_denoise.h, csrc/art_shade.h) compiled by g++.  The argument rules are the ABI's (include/art_hip.h); pointers are host
// memory; out3f may be color3f.  With -DSVGF_HOST_MAIN the file is a program that runs both over inputs of its own and checks what can
// be checked without a reference (the sanitizer build's target).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "art_hip.h"
#include "../denoise_host/filter_host.h"
#include "../../ada-ray-tracer_amd/csrc/art_shade.h"

using namespace art;

extern "C" int sh_denoise_svgf(const ArtSvgfParams* p, const float* color3f, const float* moments2f, const float* albedo3f, const float* normal3f,
                               const float* depth, float* out3f, float* variance_out) {
  dn::Params P;
  if (dn::params_from_abi(p, color3f, moments2f, albedo3f, normal3f, depth, out3f, false, P)) return 1;      // (the library's own derivation and refusals)
  filter_host<dn::Mode::Svgf>(P, p->iterations, p->n_colours, color3f, moments2f, albedo3f, normal3f, depth, out3f, variance_out);
  return 0;
}

// One batch: rad planes [3][samples][npix] (r, g, b), the frame's background, pixmap (npix entries) or null = identity.  accum and moments
// take accumulate_pixel_moments' update, accum_plain accumulate_pixel's.
extern "C" int sh_accumulate(int32_t npix, int32_t samples, int32_t aa_on, const float* rad, const float* background3, const uint32_t* pixmap,
                             float* accum, float* moments, float* accum_plain) {
  if (npix < 0 || samples < 0 || !rad || !background3 || !accum || !moments || !accum_plain) return 1;
  DevFrame f; std::memset(&f, 0, sizeof f);
  f.aa_on = aa_on; std::memcpy(f.background, background3, 12);
  DevPaths q; std::memset(&q, 0, sizeof q);
  const size_t plane = (size_t)samples * (size_t)npix;
  q.P = samples * npix; q.npix = npix; q.pixmap = pixmap;
  q.rad_r = const_cast<float*>(rad); q.rad_g = const_cast<float*>(rad) + plane; q.rad_b = const_cast<float*>(rad) + 2 * plane;
  for (int pl = 0; pl < npix; ++pl) {
    accumulate_pixel_moments(f, q, pl, samples, accum, moments);
    accumulate_pixel(f, q, pl, samples, accum_plain);
  }
  return 0;
}

#ifdef SVGF_HOST_MAIN
static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }
static float uni(uint32_t& s) { return (float)lcg(s) * (1.0f / 16777216.0f); }

int main() {
  uint32_t seed = 12345u;
  int bad = 0;
  // the accumulate: three batches over a sharded pixel list, anti-aliasing on and off; both accums must be the same bits
  for (int aa = 0; aa < 2; ++aa) {
    const int npix = 37, samples = 8, frame = 100;
    std::vector<uint32_t> pm(npix);
    for (int k = 0; k < npix; ++k) pm[k] = (uint32_t)(frame - 1 - 2 * k);
    std::vector<float> accum(3 * frame, 0.0f), plain(3 * frame, 0.0f), mom(2 * frame, 0.0f), rad(3 * (size_t)samples * npix);
    const float bg[3] = {0.125f, 0.25f, 0.5f};
    for (int b = 0; b < 3; ++b) {
      for (float& v : rad) v = uni(seed) * 3.0f;
      if (sh_accumulate(npix, samples, aa, rad.data(), bg, pm.data(), accum.data(), mom.data(), plain.data())) { std::puts("sh_accumulate refused"); return 1; }
    }
    if (std::memcmp(accum.data(), plain.data(), accum.size() * 4)) { std::printf("aa %d: the accum with moments differs from the plain accum\n", aa); ++bad; }
    for (int k = 0; k < frame; ++k) {
      const bool owned = (k & 1) == ((frame - 1) & 1) && (frame - 1 - k) / 2 < npix;
      if (!owned && (mom[2 * k] != 0.0f || mom[2 * k + 1] != 0.0f || accum[3 * k] != 0.0f)) { std::printf("aa %d: pixel %d is not owned and was written\n", aa, k); ++bad; }
      if (owned && !(mom[2 * k] > 0.0f && mom[2 * k + 1] > 0.0f)) { std::printf("aa %d: pixel %d has no moments\n", aa, k); ++bad; }
    }
  }
  // the filter: sizes around the image border, every guide, non-finite entries; the output must be finite where a finite neighbour exists
  const int sizes[][2] = {{1, 1}, {1, 9}, {9, 1}, {7, 5}, {37, 23}};
  for (const auto& wh : sizes) {
    const int W = wh[0], H = wh[1]; const size_t N = (size_t)W * H;
    std::vector<float> color(3 * N), mom(2 * N), alb(3 * N), nrm(3 * N), dep(N), out(3 * N), var(N);
    for (size_t k = 0; k < N; ++k) {
      for (int c = 0; c < 3; ++c) { color[3 * k + c] = 4.0f * uni(seed); alb[3 * k + c] = uni(seed); nrm[3 * k + c] = (c == 2) ? 1.0f : 0.0f; }
      const float l = dn::lum3(color[3 * k], color[3 * k + 1], color[3 * k + 2]);
      mom[2 * k] = l; mom[2 * k + 1] = l * l / 4.0f * (1.0f + uni(seed));
      dep[k] = 5.0f + 0.1f * (float)(k % W) + 0.01f * uni(seed);
    }
    if (N > 3) { color[3] = NAN; mom[2 * 2] = INFINITY; dep[N - 1] = NAN; }
    for (int it = 1; it <= 8; it += 3) {
      ArtSvgfParams p = {W, H, it, 1, 7, 4, 0.25f, 4.0f, 1.0f};
      if (sh_denoise_svgf(&p, color.data(), mom.data(), alb.data(), nrm.data(), dep.data(), out.data(), var.data())) { std::puts("sh_denoise_svgf refused"); return 1; }
      for (size_t k = 0; k < N; ++k) {
        if (N > 3 && k != N - 1 && !std::isfinite(out[3 * k])) { std::printf("%d x %d, %d iterations: pixel %zu is not finite\n", W, H, it, k); ++bad; }
        if (!(var[k] >= 0.0f)) { std::printf("%d x %d, %d iterations: variance of pixel %zu is %g\n", W, H, it, k, var[k]); ++bad; }
      }
    }
    ArtSvgfParams r = {W, H, 1, 1, 7, 1, 0.25f, 4.0f, 1.0f};
    if (!sh_denoise_svgf(&r, color.data(), mom.data(), nullptr, nullptr, nullptr, out.data(), nullptr)) { std::puts("n_colours 1 was accepted"); ++bad; }
  }
  std::printf("svgf_host: %s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
#endif
