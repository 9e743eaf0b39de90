// TEST-ONLY: the text of art_auto_exposure_device and art_display_device (csrc/art_display.h) compiled by g++ as a stand-alone program.
//   display_host                    its own checks (the refusals of params_from_abi, a few values by hand); prints "display_host: ok"
//   display_host exposure IN OUT    IN:  ArtExposureParams (11 words), the state (260 words), color (3 floats per pixel, row-major)
//                                   OUT: the state after the call (260 words)
//   display_host display IN OUT     IN:  ArtDisplayParams (9 words), has_state and want (int32: bit 0 screen, bit 1 ldr), the state (260
//                                        words, read when has_state), color
//                                   OUT: screen (1 word per pixel) if wanted, then ldr (3 floats per pixel) if wanted, in p.layout
// tests/test_display_reference_host.py holds OUT to tests/display_ref.py bit for bit.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "art_display.h"

using namespace art;

static int fail(const char* what) { std::fprintf(stderr, "display_host: %s\n", what); return 1; }

// the two kernels of art_display.hip over arrays: zero the bins, count every pixel, walk the bins
static void run_exposure(const dp::ExposureParams& P, const float* color, uint32_t* state) {
  for (int i = 0; i < dp::kBins; ++i) state[4 + i] = 0u;
  const size_t N = (size_t)P.W * (size_t)P.H;
  for (size_t p = 0; p < N; ++p) state[4 + dp::exposure_bin(P, color, p)] += 1u;
  dp::exposure_from_histogram(P, state);
}

static void run_display(const dp::DisplayParams& P, const float* color, const uint32_t* state, uint32_t* screen, float* ldr) {
  const float e = state ? __builtin_bit_cast(float, state[0]) : P.exposure;
  for (int y = 0; y < P.H; ++y)
    for (int x = 0; x < P.W; ++x) dp::display_pixel(P, color, e, screen, ldr, x, y);
}

static bool refused(const ArtExposureParams& p, const void* c, const void* s, const char* text) {
  dp::ExposureParams P;
  const char* why = dp::params_from_abi(&p, c, s, P);
  return why && std::strstr(why, text);
}
static bool refused(const ArtDisplayParams& p, const void* c, const void* st, const void* s, const void* l, const char* text) {
  dp::DisplayParams P;
  const char* why = dp::params_from_abi(&p, c, st, s, l, P);
  return why && std::strstr(why, text);
}

static int self_check() {
  const ArtExposureParams eg = {2, 1, 1.0f, -12.0f, 4.0f, 0.0f, 1.0f, 0.18f, 1.0f, 1e-3f, 1e3f};
  std::vector<float> color(6, 0.0f), ldr(6);
  std::vector<uint32_t> state(dp::kStateWords, 0u), screen(2);
  dp::ExposureParams EP;
  if (dp::params_from_abi(&eg, color.data(), state.data(), EP)) return fail("a good exposure call is refused");
  if (dp::params_from_abi((const ArtExposureParams*)nullptr, color.data(), state.data(), EP) == nullptr) return fail("null ArtExposureParams");
  if (!refused(eg, nullptr, state.data(), "null color3f or state") || !refused(eg, color.data(), nullptr, "null color3f or state")) return fail("null pointers");
  ArtExposureParams b = eg; b.width = 0;
  if (!refused(b, color.data(), state.data(), "width and height")) return fail("width");
  b = eg; b.width = 1 << 15; b.height = 1 << 14;
  if (!refused(b, color.data(), state.data(), "2^28")) return fail("size");
  b = eg; b.scale = INFINITY;
  if (!refused(b, color.data(), state.data(), "scale")) return fail("scale");
  b = eg; b.min_log2 = 4.0f;
  if (!refused(b, color.data(), state.data(), "min_log2")) return fail("min_log2 = max_log2");
  b = eg; b.max_log2 = NAN;
  if (!refused(b, color.data(), state.data(), "min_log2")) return fail("max_log2 NaN");
  b = eg; b.min_log2 = -127.0f;
  if (!refused(b, color.data(), state.data(), "min_log2")) return fail("min_log2 -127");
  b = eg; b.low_fraction = 0.5f; b.high_fraction = 0.5f;
  if (!refused(b, color.data(), state.data(), "fractions")) return fail("equal fractions");
  b = eg; b.low_fraction = -0.1f;
  if (!refused(b, color.data(), state.data(), "fractions")) return fail("low_fraction < 0");
  b = eg; b.high_fraction = 1.5f;
  if (!refused(b, color.data(), state.data(), "fractions")) return fail("high_fraction > 1");
  b = eg; b.high_fraction = NAN;
  if (!refused(b, color.data(), state.data(), "fractions")) return fail("high_fraction NaN");
  b = eg; b.key = 0.0f;
  if (!refused(b, color.data(), state.data(), "key")) return fail("key");
  b = eg; b.min_exposure = 0.0f;
  if (!refused(b, color.data(), state.data(), "exposure bounds")) return fail("min_exposure");
  b = eg; b.max_exposure = 1e-4f;
  if (!refused(b, color.data(), state.data(), "exposure bounds")) return fail("max_exposure < min_exposure");
  b = eg; b.adapt = 0.0f;
  if (!refused(b, color.data(), state.data(), "adapt")) return fail("adapt 0");
  b = eg; b.adapt = 1.5f;
  if (!refused(b, color.data(), state.data(), "adapt")) return fail("adapt 1.5");
  b = eg; b.adapt = NAN;
  if (!refused(b, color.data(), state.data(), "adapt")) return fail("adapt NaN");
  if (!refused(eg, color.data(), (const char*)state.data() + 1, "aligned")) return fail("alignment");
  if (!refused(eg, color.data(), color.data() + 5, "overlaps")) return fail("state over color3f");
  // by hand: two grey pixels of luminance 0.25 and 1 to a rounding: log2 = -2 and 0, t = 158.75 and 190.5 (far from a bin edge), bins
  // 1 + 158 = 159 and 1 + 190 = 191; no trimming: the mean of the centres, and exposure = key * 2^-mean
  color = {0.25f, 0.25f, 0.25f, 1.0f, 1.0f, 1.0f};
  run_exposure(EP, color.data(), state.data());
  if (state[4 + 159] != 1u || state[4 + 191] != 1u || state[2] != 2u || state[3] != 1u || state[4] != 0u) return fail("two pixels counted");
  const double mean = 0.5 * ((-12.0 + (158.5 / 254.0) * 16.0) + (-12.0 + (190.5 / 254.0) * 16.0));
  const float m = __builtin_bit_cast(float, state[1]), e = __builtin_bit_cast(float, state[0]);
  if (m != (float)mean || std::fabs(e - 0.18f * std::exp2(-(float)mean)) > 1e-6f) return fail("two pixels' exposure");
  // an all-black frame after it keeps the exposure and the mean, counts nothing and is no frame
  color.assign(6, 0.0f);
  run_exposure(EP, color.data(), state.data());
  if (state[0] != __builtin_bit_cast(uint32_t, e) || state[1] != __builtin_bit_cast(uint32_t, m) || state[2] != 0u || state[3] != 1u || state[4] != 2u) return fail("black after a frame");
  state.assign(dp::kStateWords, 0u);
  run_exposure(EP, color.data(), state.data());
  if (state[0] != __builtin_bit_cast(uint32_t, 1.0f) || state[1] != 0u || state[2] != 0u || state[3] != 0u) return fail("black, fresh");

  const ArtDisplayParams dg = {2, 1, 1.0f, 1.0f, ART_CURVE_LINEAR, ART_TRANSFER_SQRT, 4.0f, 0, ART_LAYOUT_ROW_MAJOR};
  dp::DisplayParams DP;
  if (dp::params_from_abi(&dg, color.data(), nullptr, screen.data(), ldr.data(), DP)) return fail("a good display call is refused");
  if (dp::params_from_abi(&dg, color.data(), state.data(), screen.data(), nullptr, DP) || dp::params_from_abi(&dg, color.data(), nullptr, nullptr, ldr.data(), DP)) return fail("one output is refused");
  if (dp::params_from_abi((const ArtDisplayParams*)nullptr, color.data(), nullptr, screen.data(), nullptr, DP) == nullptr) return fail("null ArtDisplayParams");
  if (!refused(dg, nullptr, nullptr, screen.data(), nullptr, "null color3f")) return fail("null color3f");
  if (!refused(dg, color.data(), nullptr, nullptr, nullptr, "both null")) return fail("no output");
  ArtDisplayParams d = dg; d.height = 0;
  if (!refused(d, color.data(), nullptr, screen.data(), nullptr, "width and height")) return fail("height");
  d = dg; d.scale = NAN;
  if (!refused(d, color.data(), nullptr, screen.data(), nullptr, "scale")) return fail("display scale");
  d = dg; d.curve = 4;
  if (!refused(d, color.data(), nullptr, screen.data(), nullptr, "unknown curve")) return fail("curve 4");
  d = dg; d.curve = -1;
  if (!refused(d, color.data(), nullptr, screen.data(), nullptr, "unknown curve")) return fail("curve -1");
  d = dg; d.transfer = 3;
  if (!refused(d, color.data(), nullptr, screen.data(), nullptr, "unknown transfer")) return fail("transfer");
  d = dg; d.layout = 2;
  if (!refused(d, color.data(), nullptr, screen.data(), nullptr, "unknown layout")) return fail("layout");
  d = dg; d.dither = 2;
  if (!refused(d, color.data(), nullptr, screen.data(), nullptr, "dither")) return fail("dither");
  d = dg; d.white = 0.0f;
  if (!refused(d, color.data(), nullptr, screen.data(), nullptr, "white")) return fail("white");
  d = dg; d.exposure = -1.0f;
  if (!refused(d, color.data(), nullptr, screen.data(), nullptr, "exposure")) return fail("exposure");
  if (dp::params_from_abi(&d, color.data(), state.data(), screen.data(), nullptr, DP)) return fail("with a state p->exposure is not read");
  d = dg; d.curve = ART_CURVE_REFERENCE;
  if (!refused(d, color.data(), nullptr, screen.data(), ldr.data(), "ART_CURVE_REFERENCE")) return fail("ldr3f with the reference curve");
  if (!refused(dg, color.data(), nullptr, color.data() + 5, nullptr, "screen1u overlaps color3f")) return fail("screen over color");
  if (!refused(dg, color.data(), nullptr, nullptr, color.data() + 5, "ldr3f overlaps color3f")) return fail("ldr over color");
  if (!refused(dg, color.data(), nullptr, ldr.data() + 5, ldr.data(), "ldr3f overlaps screen1u")) return fail("ldr over screen");
  if (!refused(dg, color.data(), state.data() + 1, state.data(), nullptr, "screen1u overlaps exposure_state")) return fail("screen over the state");
  if (!refused(dg, color.data(), state.data(), screen.data(), state.data() + 259, "ldr3f overlaps exposure_state")) return fail("ldr over the state");
  // by hand: linear, sqrt, no dither: 0.25 -> 0.5 -> 127.5 -> 128; 4.0 clamps to 1 -> 255; NaN, -1 and +inf are black
  if (dp::params_from_abi(&dg, color.data(), nullptr, screen.data(), ldr.data(), DP)) return fail("params");
  color = {0.25f, 4.0f, NAN, -1.0f, INFINITY, 1.0f};
  run_display(DP, color.data(), nullptr, screen.data(), ldr.data());
  if (screen[0] != (128u | 255u << 8) || screen[1] != (255u << 16) || ldr[0] != 0.5f || ldr[1] != 1.0f || ldr[2] != 0.0f || ldr[3] != 0.0f || ldr[4] != 0.0f) return fail("linear by hand");
  // the dither adds (B + 0.5) / 16 before truncation: at (0, 0) B = 0, at (1, 0) B = 8: 127.5 + 0.03125 -> 127, 127.5 + 0.53125 -> 128
  DP.dither = 1;
  color = {0.25f, 0.25f, 0.25f, 0.25f, 0.25f, 0.25f};
  run_display(DP, color.data(), nullptr, screen.data(), nullptr);
  if (screen[0] != 0x7f7f7fu || screen[1] != 0x808080u) return fail("dither by hand");
  // the reference curve is resolve_pixel
  DP.curve = ART_CURVE_REFERENCE; DP.scale = 0.5f;
  color = {0.5f, 2.0f, 8.0f, -1.0f, 0.0f, 0.02f};
  run_display(DP, color.data(), nullptr, screen.data(), nullptr);
  if (screen[0] != resolve_pixel(mk3(0.5f, 2.0f, 8.0f), 0.5f) || screen[1] != resolve_pixel(mk3(-1.0f, 0.0f, 0.02f), 0.5f)) return fail("reference curve");
  // x-major: pixel (x, y) at x * height + y
  DP.W = 1; DP.H = 2; DP.layout = ART_LAYOUT_ADA_XY;
  if (dp::display_index(DP, 0, 1) != 1) return fail("x-major index");
  DP.W = 3; DP.H = 2;
  if (dp::display_index(DP, 2, 1) != 5 || dp::display_index(DP, 1, 0) != 2) return fail("x-major index 3 x 2");
  std::printf("display_host: ok\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 1) return self_check();
  const bool exposure = argc == 4 && !std::strcmp(argv[1], "exposure"), display = argc == 4 && !std::strcmp(argv[1], "display");
  if (!exposure && !display) return fail("usage: display_host [exposure|display IN OUT]");
  FILE* f = std::fopen(argv[2], "rb");
  if (!f) return fail("cannot open IN");
  std::vector<uint32_t> state(dp::kStateWords);
  if (exposure) {
    ArtExposureParams p;
    static_assert(sizeof p == 44, "ArtExposureParams is 11 words");
    if (std::fread(&p, sizeof p, 1, f) != 1 || std::fread(state.data(), 4, state.size(), f) != state.size()) return fail("short IN (params, state)");
    if (p.width < 1 || p.height < 1 || (long long)p.width * p.height > (1ll << 24)) return fail("bad size");
    const size_t N = (size_t)p.width * (size_t)p.height;
    std::vector<float> color(3 * N);
    if (std::fread(color.data(), 4, 3 * N, f) != 3 * N) return fail("short IN (color)");
    std::fclose(f);
    dp::ExposureParams P;
    if (const char* why = dp::params_from_abi(&p, color.data(), state.data(), P)) return fail(why);
    run_exposure(P, color.data(), state.data());
    f = std::fopen(argv[3], "wb");
    if (!f) return fail("cannot open OUT");
    if (std::fwrite(state.data(), 4, state.size(), f) != state.size()) return fail("short OUT");
    std::fclose(f);
    return 0;
  }
  ArtDisplayParams p;
  static_assert(sizeof p == 36, "ArtDisplayParams is 9 words");
  int32_t has_state = 0, want = 0;
  if (std::fread(&p, sizeof p, 1, f) != 1 || std::fread(&has_state, 4, 1, f) != 1 || std::fread(&want, 4, 1, f) != 1 ||
      std::fread(state.data(), 4, state.size(), f) != state.size())
    return fail("short IN (params, state)");
  if (p.width < 1 || p.height < 1 || (long long)p.width * p.height > (1ll << 24)) return fail("bad size");
  const size_t N = (size_t)p.width * (size_t)p.height;
  std::vector<float> color(3 * N), ldr(3 * N);
  std::vector<uint32_t> screen(N);
  if (std::fread(color.data(), 4, 3 * N, f) != 3 * N) return fail("short IN (color)");
  std::fclose(f);
  uint32_t* s = (want & 1) ? screen.data() : nullptr;
  float* l = (want & 2) ? ldr.data() : nullptr;
  const uint32_t* st = has_state ? state.data() : nullptr;
  dp::DisplayParams P;
  if (const char* why = dp::params_from_abi(&p, color.data(), st, s, l, P)) return fail(why);
  run_display(P, color.data(), st, s, l);
  f = std::fopen(argv[3], "wb");
  if (!f) return fail("cannot open OUT");
  if ((s && std::fwrite(s, 4, N, f) != N) || (l && std::fwrite(l, 4, 3 * N, f) != 3 * N)) return fail("short OUT");
  std::fclose(f);
  return 0;
}
