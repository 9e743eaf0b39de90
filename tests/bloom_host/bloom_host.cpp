// TEST-ONLY: the text of art_bloom_device (csrc/art_bloom.h) compiled by g++ as a stand-alone program.
//   bloom_host              its own checks (the refusals of params_from_abi, the level sizes and the tail rule, a 2 x 2 frame by hand); prints "bloom_host: ok"
//   bloom_host run IN OUT   IN:  ArtBloomParams (11 words), given (int32: bit 0 a state, bit 1 in place: out3f is color3f), the state's
//                                first word (a float, read with bit 0), color (3 floats per pixel, row-major)
//                           OUT: out3f, bloom3f (3 floats per pixel each), then levels 1 .. M as the down sweep left them and again as
//                                the up sweep left them (4 floats per texel: the records)
// tests/test_bloom_reference_host.py holds OUT to tests/bloom_ref.py bit for bit.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "art_bloom.h"

using namespace art;

static int fail(const char* what) { std::fprintf(stderr, "bloom_host: %s\n", what); return 1; }

static bool refused(const ArtBloomParams& p, const void* c, const void* s, const void* o, const void* b, const char* text) {
  bl::Params P;
  const char* why = bl::params_from_abi(&p, c, s, o, b, P);
  return why && std::strstr(why, text);
}

static int self_check() {
  const ArtBloomParams good = {2, 2, 8, 0, 0, 1.0f, 1.0f, 0.0f, 0.0f, 0.5f, 1.0f};
  alignas(16) static float color[1200], out[1200], bloom[1200], state[260];
  bl::Params P;
  if (bl::params_from_abi(&good, color, nullptr, out, bloom, P)) return fail("a good call is refused");
  if (bl::params_from_abi(&good, color, state, color, nullptr, P)) return fail("the in-place call is refused");
  if (bl::params_from_abi(&good, color, nullptr, nullptr, bloom, P)) return fail("bloom3f alone is refused");
  if (bl::params_from_abi(nullptr, color, nullptr, out, bloom, P) == nullptr) return fail("null ArtBloomParams");
  if (!refused(good, nullptr, nullptr, out, bloom, "null color3f")) return fail("null color3f");
  if (!refused(good, color, nullptr, nullptr, nullptr, "both null")) return fail("no output");
  ArtBloomParams b = good; b.height = 0;
  if (!refused(b, color, nullptr, out, bloom, "width and height")) return fail("height");
  b = good; b.width = 1 << 15; b.height = 1 << 14;
  if (!refused(b, color, nullptr, out, bloom, "2^28")) return fail("size");
  for (int v : {0, 9, -1}) { b = good; b.levels = v; if (!refused(b, color, nullptr, out, bloom, "levels must be 1 .. 8")) return fail("levels"); }
  for (int v : {2, -1}) { b = good; b.karis = v; if (!refused(b, color, nullptr, out, bloom, "karis must be 0 or 1")) return fail("karis"); }
  for (int v : {2, -1}) { b = good; b.variant = v; if (!refused(b, color, nullptr, out, bloom, "variant must be 0 or 1")) return fail("variant"); }
  for (float v : {(float)INFINITY, (float)NAN}) { b = good; b.scale = v; if (!refused(b, color, nullptr, out, bloom, "scale is not finite")) return fail("scale"); }
  for (float v : {(float)INFINITY, (float)NAN, -0.5f}) {
    b = good; b.threshold = v; if (!refused(b, color, nullptr, out, bloom, "threshold must be finite and not negative")) return fail("threshold");
    b = good; b.knee = v; if (!refused(b, color, nullptr, out, bloom, "knee must be finite and not negative")) return fail("knee");
    b = good; b.exposure = v; if (!refused(b, color, nullptr, out, bloom, "exposure must be finite and not negative")) return fail("exposure");
    if (bl::params_from_abi(&b, color, state, out, bloom, P)) return fail("with a state the exposure is not looked at");
  }
  for (float v : {(float)NAN, -0.25f, 1.5f}) {
    b = good; b.scatter = v; if (!refused(b, color, nullptr, out, bloom, "scatter must be in [0, 1]")) return fail("scatter");
    b = good; b.strength = v; if (!refused(b, color, nullptr, out, bloom, "strength must be in [0, 1]")) return fail("strength");
  }
  if (!refused(good, color, nullptr, color + 3, bloom, "out3f overlaps color3f")) return fail("out3f one pixel into color3f");
  if (!refused(good, color, nullptr, out, color, "bloom3f overlaps color3f")) return fail("bloom3f is color3f");
  if (!refused(good, color, nullptr, out, out + 9, "bloom3f overlaps out3f")) return fail("bloom3f into out3f");
  if (!refused(good, color, nullptr, color, color, "bloom3f overlaps color3f")) return fail("both outputs are color3f");
  if (!refused(good, color, state, state + 1, bloom, "out3f overlaps exposure_state")) return fail("out3f into the state");
  if (!refused(good, color, state, out, state + 259, "bloom3f overlaps exposure_state")) return fail("bloom3f over the state's last word");
  // the levels: 300 x 120 -> 150 x 60, 75 x 30, 38 x 15, 19 x 8, 10 x 4, 5 x 2, 3 x 1, 2 x 1; the tail from level 2 (3027 records)
  // (planes of these sizes are not needed: params_from_abi dereferences nothing, so three addresses far apart stand for them)
  const float* far_c = (const float*)((uintptr_t)1 << 32); float* far_o = (float*)((uintptr_t)2 << 32); float* far_b = (float*)((uintptr_t)3 << 32);
  b = good; b.width = 300; b.height = 120;
  if (bl::params_from_abi(&b, far_c, nullptr, far_o, far_b, P)) return fail("300 x 120 is refused");
  if (P.made != 8 || P.w[3] != 38 || P.h[3] != 15 || P.w[8] != 2 || P.h[8] != 1 || P.off[2] != 9000 || P.off[9] != 9000 + 3027 || P.tail != 2) return fail("the levels of 300 x 120");
  b.variant = 1;
  if (bl::params_from_abi(&b, far_c, nullptr, far_o, far_b, P) || P.tail != 0 || P.made != 8) return fail("variant 1 has no tail");
  b = good; b.width = 3; b.height = 5;        // 2 x 3, 1 x 2, 1 x 1: three levels whatever is asked for
  if (bl::params_from_abi(&b, far_c, nullptr, far_o, far_b, P) || P.made != 3 || P.off[4] != 9 || P.tail != 1) return fail("the levels of 3 x 5");
  b.levels = 1;                                // one level: nothing follows it, no tail
  if (bl::params_from_abi(&b, far_c, nullptr, far_o, far_b, P) || P.made != 1 || P.tail != 0) return fail("one level");
  b = good; b.width = 1920; b.height = 1080; b.levels = 6;      // 960 x 540 .. 60 x 34 (level 5), 30 x 17
  if (bl::params_from_abi(&b, far_c, nullptr, far_o, far_b, P) || P.made != 6 || P.w[5] != 60 || P.h[5] != 34 || P.tail != 5) return fail("the levels of 1920 x 1080");
  b.levels = 4;                                // level 4 is 120 x 68 = 8160 records: nothing fits
  if (bl::params_from_abi(&b, far_c, nullptr, far_o, far_b, P) || P.made != 4 || P.tail != 0) return fail("no level fits");
  // by hand (tests/test_bloom_reference_host.py states the case): 2 x 2, red = 8 0 / 0 0, one level: D_1 = 2; up(U_1) = 2 everywhere;
  // strength 1: out = s + (2 - s) = 2
  if (bl::params_from_abi(&good, color, nullptr, out, bloom, P) || P.made != 1) return fail("2 x 2");
  std::memset(color, 0, sizeof color);
  color[0] = 8.0f;
  bl::Rec4 pyr[1], dn[1];
  bl::run_host(P, color, 1.0f, pyr, dn, out, bloom);
  if (pyr[0].x != 2.0f || pyr[0].y != 0.0f || dn[0].x != 2.0f) return fail("2 x 2 by hand: the level");
  for (int k = 0; k < 4; ++k) if (out[3 * k] != 2.0f || bloom[3 * k] != 2.0f || out[3 * k + 1] != 0.0f || bloom[3 * k + 2] != 0.0f) return fail("2 x 2 by hand");
  // the soft knee, threshold 1, knee 0.5, e = 1: nothing below threshold - knee, (l - 1) / l far above (the three luminance weights need
  // not sum to exactly 1, so that factor is held between bounds)
  b = good; b.threshold = 1.0f; b.knee = 0.5f;
  if (bl::params_from_abi(&b, color, nullptr, out, bloom, P) || !P.prefilter) return fail("prefilter");
  if (bl::knee_factor(P, 1.0f, bl::T3{0.25f, 0.25f, 0.25f}) != 0.0f) return fail("below the knee nothing passes");
  if (bl::knee_factor(P, 1.0f, bl::T3{0.0f, 0.0f, 0.0f}) != 0.0f || bl::knee_factor(P, (float)NAN, bl::T3{1.0f, 1.0f, 1.0f}) != 0.0f) return fail("no luminance");
  const float f = bl::knee_factor(P, 1.0f, bl::T3{64.0f, 64.0f, 64.0f});       // l = 64 up to an ulp: 63 / 64 = 0.984375
  if (!(f > 0.98437f && f < 0.98438f)) return fail("far above the knee");
  if (bl::knee_factor(P, 1.0f, bl::T3{1.0f, 1.0f, 1.0f}) >= 0.2f || !(bl::knee_factor(P, 1.0f, bl::T3{1.0f, 1.0f, 1.0f}) > 0.1f)) return fail("on the knee: 0.125 at l = 1");
  std::printf("bloom_host: ok\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 1) return self_check();
  if (argc != 4 || std::strcmp(argv[1], "run")) return fail("usage: bloom_host [run IN OUT]");
  FILE* f = std::fopen(argv[2], "rb");
  if (!f) return fail("cannot open IN");
  ArtBloomParams p;
  static_assert(sizeof p == 44, "ArtBloomParams is 11 words");
  int32_t given = 0;
  float e0 = 0.0f;
  if (std::fread(&p, sizeof p, 1, f) != 1 || std::fread(&given, 4, 1, f) != 1 || std::fread(&e0, 4, 1, f) != 1) return fail("short IN (params)");
  if (p.width < 1 || p.height < 1 || (long long)p.width * p.height > (1ll << 24)) return fail("bad size");
  const size_t N = (size_t)p.width * (size_t)p.height;
  const bool has_state = given & 1, in_place = given & 2;
  std::vector<float> color(3 * N), out(3 * N), bloom(3 * N);
  std::vector<uint32_t> state(260, 0u);
  state[0] = __builtin_bit_cast(uint32_t, e0);
  if (std::fread(color.data(), 4, 3 * N, f) != 3 * N) return fail("short IN (color)");
  std::fclose(f);
  float* o = in_place ? color.data() : out.data();
  bl::Params P;
  if (const char* why = bl::params_from_abi(&p, color.data(), has_state ? state.data() : nullptr, o, bloom.data(), P)) return fail(why);
  const size_t R = P.off[P.made + 1];
  std::vector<bl::Rec4> pyr(R), down(R);         // (exactly the records the call needs: AddressSanitizer sees a step past them)
  bl::run_host(P, color.data(), has_state ? __builtin_bit_cast(float, state[0]) : P.exposure, pyr.data(), down.data(), o, bloom.data());
  f = std::fopen(argv[3], "wb");
  if (!f) return fail("cannot open OUT");
  if (std::fwrite(o, 4, 3 * N, f) != 3 * N || std::fwrite(bloom.data(), 4, 3 * N, f) != 3 * N || std::fwrite(down.data(), 16, R, f) != R ||
      std::fwrite(pyr.data(), 16, R, f) != R)
    return fail("short OUT");
  if (std::fclose(f)) return fail("cannot close OUT");
  return 0;
}
