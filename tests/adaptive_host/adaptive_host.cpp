// TEST-ONLY: the per-pixel text of art_adaptive_estimate_device (csrc/art_adaptive.h) compiled by g++ as a stand-alone program.
//   adaptive_host                 its own checks (the refusals of params_from_abi, a few pixels by hand); prints "adaptive_host: ok"
//   adaptive_host IN OUT          IN:  7 words {width, height, aa_on, min_colours, max_samples (int32), threshold, lum_floor (float)}, then
//                                      accum (3 floats per pixel), moments (2 floats), counts (1 uint32), row-major
//                                 OUT: mean (3 floats per pixel), variance, error (1 float each), mask (1 byte each)
// tests/test_adaptive_reference_host.py holds OUT to tests/adaptive_ref.py bit for bit.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "art_adaptive.h"

using namespace art;

static int fail(const char* what) { std::fprintf(stderr, "adaptive_host: %s\n", what); return 1; }

static bool refused(const ArtAdaptiveParams* p, const void* a, const void* m, const void* c, const void* o, const char* text) {
  ad::Params P;
  const char* why = ad::params_from_abi(p, a, m, c, o, nullptr, nullptr, nullptr, P);
  return why && std::strstr(why, text);
}

static int self_check() {
  const ArtAdaptiveParams good = {4, 3, 1, 2, 64, 0.05f, 0.01f};
  int x = 0; const void* one = &x;
  ad::Params P;
  if (ad::params_from_abi(&good, one, one, one, one, nullptr, nullptr, nullptr, P)) return fail("a good call is refused");
  if (P.n != 12 || P.per != 4 || P.min_colours != 2u || P.max_samples != 64u) return fail("Params");
  if (!refused(nullptr, one, one, one, one, "null ArtAdaptiveParams")) return fail("null params");
  if (!refused(&good, nullptr, one, one, one, "null accum3f")) return fail("null accum");
  if (!refused(&good, one, nullptr, one, one, "null accum3f")) return fail("null moments");
  if (!refused(&good, one, one, nullptr, one, "null accum3f")) return fail("null counts");
  if (!refused(&good, one, one, one, nullptr, "no output")) return fail("no output");
  ArtAdaptiveParams b = good; b.width = 0;
  if (!refused(&b, one, one, one, one, "width")) return fail("width");
  b = good; b.width = 1 << 15; b.height = 1 << 14;
  if (!refused(&b, one, one, one, one, "2^28")) return fail("size");
  b = good; b.min_colours = 1;
  if (!refused(&b, one, one, one, one, "min_colours")) return fail("min_colours");
  b = good; b.max_samples = -1;
  if (!refused(&b, one, one, one, one, "max_samples")) return fail("max_samples");
  b = good; b.threshold = NAN;
  if (!refused(&b, one, one, one, one, "threshold")) return fail("threshold");
  b = good; b.lum_floor = -0.5f;
  if (!refused(&b, one, one, one, one, "lum_floor")) return fail("negative floor");
  b = good; b.lum_floor = INFINITY;
  if (!refused(&b, one, one, one, one, "lum_floor")) return fail("infinite floor");
  // by hand, no anti-aliasing: two colours 1 and 3 (S1 = 4, S2 = 10): D = 10 - 16 / 2 = 2, v = (2 * 2) / 2 = 2, m = 2, error = sqrt(2) / 2
  P.per = 1; P.min_colours = 2; P.max_samples = 64; P.threshold = 0.5f; P.lum_floor = 0.0f; P.n = 1;
  const float acc[3] = {2.0f, 4.0f, 6.0f}, mom[2] = {4.0f, 10.0f};
  uint32_t cnt = 2;
  ad::Out o = ad::adaptive_pixel(P, acc, mom, &cnt, 0);
  if (o.mean[0] != 1.0f || o.mean[1] != 2.0f || o.mean[2] != 3.0f || o.variance != 2.0f || o.error != (float)(std::sqrt(2.0) / 2.0) || o.mask != 1) return fail("two colours");
  P.threshold = o.error;
  if (ad::adaptive_pixel(P, acc, mom, &cnt, 0).mask != 0) return fail("an error equal to the threshold is converged");
  cnt = 0; o = ad::adaptive_pixel(P, acc, mom, &cnt, 0);
  if (o.mean[0] != 0.0f || std::signbit(o.mean[0]) || !std::isinf(o.variance) || !std::isinf(o.error) || o.mask != 1) return fail("s = 0");
  cnt = 1; o = ad::adaptive_pixel(P, acc, mom, &cnt, 0);
  if (o.mean[1] != 4.0f || !std::isinf(o.variance) || o.mask != 1) return fail("n = 1");
  cnt = 64; const float nanmom[2] = {NAN, 1.0f};
  o = ad::adaptive_pixel(P, acc, nanmom, &cnt, 0);
  if (!std::isnan(o.error) || o.mask != 0) return fail("a NaN error is bounded by max_samples");
  cnt = 63; if (ad::adaptive_pixel(P, acc, nanmom, &cnt, 0).mask != 1) return fail("a NaN error keeps selecting");
  std::printf("adaptive_host: ok\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 1) return self_check();
  if (argc != 3) return fail("usage: adaptive_host [IN OUT]");
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return fail("cannot open IN");
  ArtAdaptiveParams p;
  static_assert(sizeof p == 28, "ArtAdaptiveParams is 7 words");
  if (std::fread(&p, sizeof p, 1, f) != 1) return fail("short IN (params)");
  if (p.width < 1 || p.height < 1 || (long long)p.width * p.height > (1ll << 24)) return fail("bad size");
  const size_t N = (size_t)p.width * (size_t)p.height;
  std::vector<float> accum(3 * N), mom(2 * N), mean(3 * N), var(N), err(N);
  std::vector<uint32_t> counts(N);
  std::vector<uint8_t> mask(N);
  if (std::fread(accum.data(), 4, 3 * N, f) != 3 * N || std::fread(mom.data(), 4, 2 * N, f) != 2 * N || std::fread(counts.data(), 4, N, f) != N) return fail("short IN (planes)");
  std::fclose(f);
  ad::Params P;
  if (const char* why = ad::params_from_abi(&p, accum.data(), mom.data(), counts.data(), mean.data(), var.data(), err.data(), mask.data(), P)) return fail(why);
  for (size_t q = 0; q < N; ++q) {
    const ad::Out o = ad::adaptive_pixel(P, accum.data(), mom.data(), counts.data(), q);
    mean[3 * q] = o.mean[0]; mean[3 * q + 1] = o.mean[1]; mean[3 * q + 2] = o.mean[2];
    var[q] = o.variance; err[q] = o.error; mask[q] = o.mask;
  }
  f = std::fopen(argv[2], "wb");
  if (!f) return fail("cannot open OUT");
  if (std::fwrite(mean.data(), 4, 3 * N, f) != 3 * N || std::fwrite(var.data(), 4, N, f) != N || std::fwrite(err.data(), 4, N, f) != N || std::fwrite(mask.data(), 1, N, f) != N) return fail("short OUT");
  std::fclose(f);
  return 0;
}
