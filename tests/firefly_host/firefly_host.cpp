// TEST-ONLY: the text of art_firefly_device (csrc/art_firefly.h) compiled by g++ as a stand-alone program.
//   firefly_host              its own checks (the refusals of params_from_abi and overlap_refusal, a 3 x 3 frame by hand); prints "firefly_host: ok"
//   firefly_host run IN OUT   IN:  ArtFireflyParams (8 words), given (int32: bit 0 moments, bit 1 id, bit 2 in place: out3f is color3f and
//                                  moments_out2f is moments2f), color (3 floats per pixel), then the moments (2 floats per pixel) and the id
//                                  (1 int32 per pixel) where given, row-major
//                             OUT: out3f (3 floats per pixel), moments_out2f where given (2 floats per pixel), clamped1b (1 byte per pixel)
// tests/test_firefly_reference_host.py holds OUT to tests/firefly_ref.py bit for bit.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "art_firefly.h"

using namespace art;

static int fail(const char* what) { std::fprintf(stderr, "firefly_host: %s\n", what); return 1; }

// the two kernels of art_firefly.hip over arrays
static void run(const fi::Params& P, const float* color, const float* moments, const int32_t* id, float* out, float* moments_out, uint8_t* clamped) {
  std::vector<float> keys((size_t)P.W * (size_t)P.H);
  if (P.radius == 1) {
    if (id) fi::run_host<1, true>(P, color, moments, id, keys.data(), out, moments_out, clamped);
    else fi::run_host<1, false>(P, color, moments, id, keys.data(), out, moments_out, clamped);
  } else {
    if (id) fi::run_host<2, true>(P, color, moments, id, keys.data(), out, moments_out, clamped);
    else fi::run_host<2, false>(P, color, moments, id, keys.data(), out, moments_out, clamped);
  }
}

static bool refused(const ArtFireflyParams& p, const void* c, const void* m, const void* o, const void* mo, const char* text) {
  fi::Params P;
  const char* why = fi::params_from_abi(&p, c, m, o, mo, P);
  return why && std::strstr(why, text);
}

static int self_check() {
  const ArtFireflyParams good = {3, 3, 1, 2, 2, 1.0f, 2.0f, 0.0f};
  // green only, powers of two: l = 0.7152f * g exactly, so every key is a = 0.7152f times 1 2 1 / 4 64 2 / 1 8 1
  const float green[9] = {1, 2, 1, 4, 64, 2, 1, 8, 1};
  std::vector<float> color(27, 0.0f), out(27), mom(18), mout(18);
  std::vector<uint8_t> flag(9);
  std::vector<int32_t> id(9, 7);
  for (int k = 0; k < 9; ++k) { color[3 * k + 1] = green[k]; mom[2 * k] = green[k]; mom[2 * k + 1] = green[k] * green[k]; }
  fi::Params P;
  if (fi::params_from_abi(&good, color.data(), mom.data(), out.data(), mout.data(), P)) return fail("a good call is refused");
  if (fi::params_from_abi(&good, color.data(), mom.data(), color.data(), mom.data(), P)) return fail("the in-place call is refused");
  if (fi::params_from_abi(&good, color.data(), nullptr, out.data(), nullptr, P)) return fail("the call without moments is refused");
  if (fi::params_from_abi(nullptr, color.data(), nullptr, out.data(), nullptr, P) == nullptr) return fail("null ArtFireflyParams");
  if (!refused(good, nullptr, nullptr, out.data(), nullptr, "null color3f or out3f") || !refused(good, color.data(), nullptr, nullptr, nullptr, "null color3f or out3f")) return fail("null planes");
  if (!refused(good, color.data(), nullptr, out.data(), mout.data(), "moments_out2f is given without moments2f")) return fail("moments_out alone");
  if (!refused(good, color.data(), mom.data(), out.data(), nullptr, "moments2f is given without moments_out2f")) return fail("moments alone");
  ArtFireflyParams b = good; b.width = 0;
  if (!refused(b, color.data(), nullptr, out.data(), nullptr, "width and height")) return fail("width");
  b = good; b.width = 1 << 15; b.height = 1 << 14;
  if (!refused(b, color.data(), nullptr, out.data(), nullptr, "2^28")) return fail("size");
  for (int r : {0, 3, -1}) { b = good; b.radius = r; if (!refused(b, color.data(), nullptr, out.data(), nullptr, "radius must be 1 or 2")) return fail("radius"); }
  for (int r : {0, 5}) { b = good; b.rank = r; b.min_count = 5; if (!refused(b, color.data(), nullptr, out.data(), nullptr, "rank must be 1 .. 4")) return fail("rank"); }
  b = good; b.min_count = 1;
  if (!refused(b, color.data(), nullptr, out.data(), nullptr, "min_count")) return fail("min_count below rank");
  b = good; b.min_count = 9;
  if (!refused(b, color.data(), nullptr, out.data(), nullptr, "min_count")) return fail("min_count 9 at radius 1");
  b = good; b.radius = 2; b.min_count = 24;
  if (fi::params_from_abi(&b, color.data(), nullptr, out.data(), nullptr, P)) return fail("min_count 24 at radius 2 is refused");
  b.min_count = 25;
  if (!refused(b, color.data(), nullptr, out.data(), nullptr, "min_count")) return fail("min_count 25 at radius 2");
  for (float v : {(float)INFINITY, (float)NAN}) { b = good; b.scale = v; if (!refused(b, color.data(), nullptr, out.data(), nullptr, "scale is not finite")) return fail("scale"); }
  for (float v : {(float)INFINITY, (float)NAN, 0.5f, -2.0f}) { b = good; b.gain = v; if (!refused(b, color.data(), nullptr, out.data(), nullptr, "gain must be finite and at least 1")) return fail("gain"); }
  for (float v : {(float)INFINITY, (float)NAN, -0.5f}) { b = good; b.floor = v; if (!refused(b, color.data(), nullptr, out.data(), nullptr, "floor must be finite and at least 0")) return fail("floor"); }
  if (fi::params_from_abi(&good, color.data(), mom.data(), out.data(), mout.data(), P)) return fail("a good call is refused");
  // overlaps: the two identities pass, everything else that touches an output is refused
  if (fi::overlap_refusal(P, color.data(), mom.data(), id.data(), out.data(), mout.data(), flag.data())) return fail("no overlap is refused");
  if (fi::overlap_refusal(P, color.data(), mom.data(), id.data(), color.data(), mom.data(), flag.data())) return fail("in place is refused");
  if (fi::overlap_refusal(P, color.data(), mom.data(), color.data(), out.data(), mout.data(), nullptr)) return fail("two inputs that overlap are refused");
  if (!fi::overlap_refusal(P, color.data(), mom.data(), id.data(), color.data() + 3, mout.data(), nullptr)) return fail("out3f one pixel into color3f");
  if (!fi::overlap_refusal(P, color.data(), mom.data(), id.data(), out.data(), mom.data() + 2, nullptr)) return fail("moments_out2f one pixel into moments2f");
  if (!fi::overlap_refusal(P, color.data(), mom.data(), id.data(), mom.data(), mout.data(), nullptr)) return fail("out3f over moments2f");
  if (!fi::overlap_refusal(P, color.data(), mom.data(), id.data(), out.data(), color.data(), nullptr)) return fail("moments_out2f over color3f");
  if (!fi::overlap_refusal(P, color.data(), mom.data(), id.data(), out.data(), mout.data(), id.data())) return fail("clamped1b over id");
  if (!fi::overlap_refusal(P, color.data(), mom.data(), id.data(), out.data(), mout.data(), color.data() + 26)) return fail("clamped1b over color3f");
  if (!fi::overlap_refusal(P, color.data(), mom.data(), id.data(), out.data(), out.data() + 12, nullptr)) return fail("moments_out2f over out3f");
  if (!fi::overlap_refusal(P, color.data(), mom.data(), id.data(), out.data(), mout.data(), mout.data() + 17)) return fail("clamped1b over moments_out2f");
  // by hand (tests/test_firefly_reference_host.py states the case): rank 2, gain 2.  The centre's neighbours hold a * {1, 2, 1, 4, 2, 1, 8, 1}:
  // m = 4 a, T = 8 a, l = 64 a > T, f = 8 a / 64 a = 0.125: out = (0, 8, 0), moments (64, 4096) -> (8, 64), flag 1.  Every other pixel keeps
  // its words: e.g. the 8 below the centre sees {4, 64, 2, 1, 1}, m = 4 a, T = 8 a, and 8 a > 8 a is false.
  run(P, color.data(), mom.data(), id.data(), out.data(), mout.data(), flag.data());
  for (int k = 0; k < 9; ++k) {
    const float g = (k == 4) ? 8.0f : green[k];
    if (out[3 * k] != 0.0f || out[3 * k + 1] != g || out[3 * k + 2] != 0.0f || mout[2 * k] != g || mout[2 * k + 1] != g * g || flag[k] != (k == 4 ? 1 : 0)) return fail("3 x 3 by hand");
  }
  // rank 1: m = 8 a, T = 16 a, f = 0.25
  b = good; b.rank = 1;
  if (fi::params_from_abi(&b, color.data(), mom.data(), out.data(), mout.data(), P)) return fail("rank 1 is refused");
  run(P, color.data(), mom.data(), nullptr, out.data(), mout.data(), flag.data());
  if (out[13] != 16.0f || mout[8] != 16.0f || mout[9] != 256.0f || flag[4] != 1) return fail("3 x 3 by hand, rank 1");
  // another id at the centre: it has no neighbour, count 0 < min_count, it is kept; in place
  id[4] = 9;
  std::vector<float> c2 = color, m2 = mom;
  run(P, c2.data(), m2.data(), id.data(), c2.data(), m2.data(), flag.data());
  for (int k = 0; k < 27; ++k) if (c2[k] != color[k]) return fail("a pixel alone in its id");
  for (int k = 0; k < 9; ++k) if (flag[k] != 0) return fail("a pixel alone in its id (flag)");
  // a bad centre: flag 2, its NaN leaves as the quiet NaN, and it is nobody's neighbour (the 8 now sees {4, 2, 1, 1}: m = 4 a, T = 8 a, kept)
  c2 = color; c2[12] = -NAN;
  run(P, c2.data(), mom.data(), nullptr, out.data(), mout.data(), flag.data());
  if (flag[4] != 2 || __builtin_bit_cast(uint32_t, out[12]) != 0x7fc00000u || out[13] != 64.0f || mout[8] != 64.0f) return fail("a bad centre");
  for (int k = 0; k < 9; ++k) if (k != 4 && flag[k] != 0) return fail("a bad centre's neighbours");
  std::printf("firefly_host: ok\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 1) return self_check();
  if (argc != 4 || std::strcmp(argv[1], "run")) return fail("usage: firefly_host [run IN OUT]");
  FILE* f = std::fopen(argv[2], "rb");
  if (!f) return fail("cannot open IN");
  ArtFireflyParams p;
  static_assert(sizeof p == 32, "ArtFireflyParams is 8 words");
  int32_t given = 0;
  if (std::fread(&p, sizeof p, 1, f) != 1 || std::fread(&given, 4, 1, f) != 1) return fail("short IN (params)");
  if (p.width < 1 || p.height < 1 || (long long)p.width * p.height > (1ll << 24)) return fail("bad size");
  const size_t N = (size_t)p.width * (size_t)p.height;
  const bool has_m = given & 1, has_id = given & 2, in_place = given & 4;
  std::vector<float> color(3 * N), mom(has_m ? 2 * N : 0), out(3 * N), mout(has_m ? 2 * N : 0);
  std::vector<int32_t> id(has_id ? N : 0);
  std::vector<uint8_t> flag(N);
  if (std::fread(color.data(), 4, 3 * N, f) != 3 * N) return fail("short IN (color)");
  if (has_m && std::fread(mom.data(), 4, 2 * N, f) != 2 * N) return fail("short IN (moments)");
  if (has_id && std::fread(id.data(), 4, N, f) != N) return fail("short IN (id)");
  std::fclose(f);
  float* o = in_place ? color.data() : out.data();
  float* mo = has_m ? (in_place ? mom.data() : mout.data()) : nullptr;
  const float* m = has_m ? mom.data() : nullptr;
  const int32_t* ids = has_id ? id.data() : nullptr;
  fi::Params P;
  if (const char* why = fi::params_from_abi(&p, color.data(), m, o, mo, P)) return fail(why);
  if (const char* why = fi::overlap_refusal(P, color.data(), m, ids, o, mo, flag.data())) return fail(why);
  run(P, color.data(), m, ids, o, mo, flag.data());
  f = std::fopen(argv[3], "wb");
  if (!f) return fail("cannot open OUT");
  if (std::fwrite(o, 4, 3 * N, f) != 3 * N || (has_m && std::fwrite(mo, 4, 2 * N, f) != 2 * N) || std::fwrite(flag.data(), 1, N, f) != N) return fail("short OUT");
  if (std::fclose(f)) return fail("cannot close OUT");
  return 0;
}
