// TEST-ONLY: the per-pixel text of art_svgf_spatial_variance_device (csrc/art_svgf_spatial.h) compiled by g++ as a stand-alone program.
//   svgf_spatial_host                 its own checks (the refusals of params_from_abi, a few pixels by hand); prints "svgf_spatial_host: ok"
//   svgf_spatial_host IN OUT [inplace] IN:  6 words {width, height, radius, normal_log2 (int32), min_history, sigma_depth (float)}, then the
//                                          history (3 planes of 4 floats per pixel) and variance_in (1 float per pixel), row-major
//                                     OUT: variance_out (1 float per pixel); with "inplace" it is written over variance_in itself
// tests/test_svgf_spatial_reference_host.py holds OUT to tests/svgf_spatial_ref.py bit for bit.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "art_svgf_spatial.h"

using namespace art;

static int fail(const char* what) { std::fprintf(stderr, "svgf_spatial_host: %s\n", what); return 1; }

static bool refused(const ArtSvgfSpatialParams* p, const void* h, const void* vi, const void* vo, const char* text) {
  sv::Params P;
  const char* why = sv::params_from_abi(p, h, vi, vo, P);
  return why && std::strstr(why, text);
}

static void run(const sv::Params& P, const sv::Rec4* hist, const float* vin, float* vout) {
  for (int y = 0; y < P.H; ++y)
    for (int x = 0; x < P.W; ++x) vout[(size_t)y * P.W + x] = sv::spatial_pixel(P, hist, vin, x, y);
}

static int self_check() {
  const ArtSvgfSpatialParams good = {3, 1, 3, 0, 4.0f, 0.0f};
  std::vector<sv::Rec4> hist(9);
  std::vector<float> vin(3), vout(3);
  sv::Params P;
  if (sv::params_from_abi(&good, hist.data(), vin.data(), vout.data(), P)) return fail("a good call is refused");
  if (sv::params_from_abi(&good, hist.data(), vin.data(), vin.data(), P)) return fail("in-place output is refused");
  if (P.W != 3 || P.H != 1 || P.radius != 3 || P.normal_log2 != 0 || P.min_history != 4.0f || P.sigma_depth != 0.0f) return fail("Params");
  if (!refused(nullptr, hist.data(), vin.data(), vout.data(), "null ArtSvgfSpatialParams")) return fail("null params");
  if (!refused(&good, nullptr, vin.data(), vout.data(), "null hist")) return fail("null hist");
  if (!refused(&good, hist.data(), nullptr, vout.data(), "null hist")) return fail("null variance_in1f");
  if (!refused(&good, hist.data(), vin.data(), nullptr, "null hist")) return fail("null variance_out1f");
  ArtSvgfSpatialParams b = good; b.height = 0;
  if (!refused(&b, hist.data(), vin.data(), vout.data(), "width and height")) return fail("height");
  b = good; b.width = 1 << 15; b.height = 1 << 14;
  if (!refused(&b, hist.data(), vin.data(), vout.data(), "2^28")) return fail("size");
  b = good; b.radius = 0;
  if (!refused(&b, hist.data(), vin.data(), vout.data(), "radius")) return fail("radius 0");
  b = good; b.radius = 4;
  if (!refused(&b, hist.data(), vin.data(), vout.data(), "radius")) return fail("radius 4");
  b = good; b.normal_log2 = -1;
  if (!refused(&b, hist.data(), vin.data(), vout.data(), "normal_log2")) return fail("normal_log2 -1");
  b = good; b.normal_log2 = 11;
  if (!refused(&b, hist.data(), vin.data(), vout.data(), "normal_log2")) return fail("normal_log2 11");
  b = good; b.min_history = NAN;
  if (!refused(&b, hist.data(), vin.data(), vout.data(), "NaN")) return fail("min_history");
  b = good; b.sigma_depth = NAN;
  if (!refused(&b, hist.data(), vin.data(), vout.data(), "NaN")) return fail("sigma_depth");
  if (!refused(&good, hist.data(), vin.data(), (float*)hist.data() + 35, "overlaps hist")) return fail("overlap at the end of hist");
  if (!refused(&good, (const char*)hist.data() + 4, vin.data(), hist.data(), "overlaps hist")) return fail("overlap at the start of hist");
  // by hand: three pixels of one colour each with luminances 1, 2, 3, equal normals, no depth stop: every weight is 1, N = 3,
  // M1 = 2, M2 = 14 / 3, D = 2 / 3, variance = (2 / 3) * (3 / 2) / 1 = 1 at each of them
  for (int k = 0; k < 3; ++k) {
    const float l = (float)(k + 1);
    hist[k] = {l, l, l, 1.0f}; hist[3 + k] = {l, l * l, 5.0f, 0.0f}; hist[6 + k] = {0.0f, 0.0f, 1.0f, 0.0f};
    vin[k] = INFINITY;
  }
  run(P, hist.data(), vin.data(), vout.data());
  for (int k = 0; k < 3; ++k) if (std::fabs(vout[k] - 1.0f) > 1e-6f) return fail("three colours pooled");
  // a long pixel keeps its word; its neighbours still pool it
  hist[1].w = 8.0f; vin[1] = 0.125f;
  run(P, hist.data(), vin.data(), vout.data());
  if (vout[1] != 0.125f || !(vout[0] > 0.0f) || !std::isfinite(vout[0])) return fail("a long pixel");
  // alone in its window (the neighbours' normals are orthogonal): one colour gives +infinity, two colours give temporal's variance
  hist[1].w = 1.0f; vin[1] = INFINITY; hist[6] = {1.0f, 0.0f, 0.0f, 0.0f}; hist[8] = {0.0f, 1.0f, 0.0f, 0.0f};
  run(P, hist.data(), vin.data(), vout.data());
  if (!std::isinf(vout[1]) || vout[1] < 0.0f) return fail("one colour alone");
  hist[1].w = 2.0f; hist[4] = {2.0f, 5.0f, 5.0f, 0.0f};
  run(P, hist.data(), vin.data(), vout.data());
  if (vout[1] != (float)(((5.0 - 4.0) * (2.0 / 1.0)) / 2.0)) return fail("two colours alone");
  // a NaN leaves as the quiet NaN
  hist[1].w = -2.0f; hist[0].w = 2.0f; hist[6] = {0.0f, 0.0f, 1.0f, 0.0f}; hist[4].y = 5.0f; hist[3].y = -1e30f;
  run(P, hist.data(), vin.data(), vout.data());
  for (int k = 0; k < 3; ++k) if (vout[k] != vout[k] && __builtin_bit_cast(uint32_t, vout[k]) != 0x7fc00000u) return fail("a NaN that is not the quiet NaN");
  std::printf("svgf_spatial_host: ok\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 1) return self_check();
  if (argc != 3 && !(argc == 4 && !std::strcmp(argv[3], "inplace"))) return fail("usage: svgf_spatial_host [IN OUT [inplace]]");
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return fail("cannot open IN");
  ArtSvgfSpatialParams p;
  static_assert(sizeof p == 24, "ArtSvgfSpatialParams is 6 words");
  if (std::fread(&p, sizeof p, 1, f) != 1) return fail("short IN (params)");
  if (p.width < 1 || p.height < 1 || (long long)p.width * p.height > (1ll << 24)) return fail("bad size");
  const size_t N = (size_t)p.width * (size_t)p.height;
  std::vector<sv::Rec4> hist(3 * N);
  std::vector<float> vin(N), vout(N);
  if (std::fread(hist.data(), 16, 3 * N, f) != 3 * N || std::fread(vin.data(), 4, N, f) != N) return fail("short IN (planes)");
  std::fclose(f);
  float* out = (argc == 4) ? vin.data() : vout.data();
  sv::Params P;
  if (const char* why = sv::params_from_abi(&p, hist.data(), vin.data(), out, P)) return fail(why);
  run(P, hist.data(), vin.data(), out);
  f = std::fopen(argv[2], "wb");
  if (!f) return fail("cannot open OUT");
  if (std::fwrite(out, 4, N, f) != N) return fail("short OUT");
  std::fclose(f);
  return 0;
}
