// TEST-ONLY: the text of art_upsample_device (csrc/art_upsample.h) compiled by g++ as a stand-alone program.
//   upsample_host              its own checks (the refusals of params_from_abi and overlap_refusal, a few values by hand); prints "upsample_host: ok"
//   upsample_host run IN OUT   IN:  one call after the other until the file ends, each: ArtUpsampleParams (11 words), given (int32: bit 0
//                                   albedo, 1 normal, 2 depth, 3 id), lo_color (3 floats per lo pixel), then for every guide given, in that
//                                   order, its lo plane and its hi plane (row-major)
//                              OUT: per call out3f (3 floats per hi pixel), then fallback1b (1 byte per hi pixel)
// tests/test_upsample_reference_host.py holds OUT to tests/upsample_ref.py bit for bit.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "art_upsample.h"

using namespace art;

static int fail(const char* what) { std::fprintf(stderr, "upsample_host: %s\n", what); return 1; }

// the two kernels of art_upsample.hip over arrays: pack every lo pixel, then every hi pixel
static void run(const us::Params& P, const float* lo_color, const ArtUpsampleGuides& lo, const ArtUpsampleGuides& hi, float* out, uint8_t* fallback) {
  const size_t NL = (size_t)P.LW * (size_t)P.LH;
  std::vector<us::Rec4> c(NL), g(NL);
  for (size_t q = 0; q < NL; ++q) us::pack_lo(P, lo_color, lo.albedo3f, lo.normal3f, lo.depth, q, c[q], g[q]);
  const us::HiGuides h = {hi.albedo3f, hi.normal3f, hi.depth, hi.id};
  for (int y = 0; y < P.H; ++y)
    for (int x = 0; x < P.W; ++x) {
      const size_t p = (size_t)y * (size_t)P.W + (size_t)x;
      float* o = out + 3 * p;
      uint8_t fb;
      if (P.footprint == 2) {
        if (P.has_id) us::upsample_pixel<2, true>(P, c.data(), g.data(), lo.id, h, x, y, o[0], o[1], o[2], fb);
        else us::upsample_pixel<2, false>(P, c.data(), g.data(), nullptr, h, x, y, o[0], o[1], o[2], fb);
      } else {
        if (P.has_id) us::upsample_pixel<4, true>(P, c.data(), g.data(), lo.id, h, x, y, o[0], o[1], o[2], fb);
        else us::upsample_pixel<4, false>(P, c.data(), g.data(), nullptr, h, x, y, o[0], o[1], o[2], fb);
      }
      if (fallback) fallback[p] = fb;
    }
}

static bool refused(const ArtUpsampleParams& p, const void* c, const ArtUpsampleGuides* lo, const ArtUpsampleGuides* hi, const void* out, const char* text) {
  us::Params P;
  const char* why = us::params_from_abi(&p, c, lo, hi, out, P);
  return why && std::strstr(why, text);
}

static int self_check() {
  const ArtUpsampleParams good = {4, 2, 2, 1, 2, 0, 5, 1.0f, 1.0f, {0.0f, 0.0f}};
  std::vector<float> lo_color = {1.0f, 2.0f, 4.0f, 3.0f, 6.0f, 12.0f}, out(24), plane(24, 0.5f);
  std::vector<uint8_t> fb(8);
  const ArtUpsampleGuides none = {nullptr, nullptr, nullptr, nullptr};
  us::Params P;
  if (us::params_from_abi(&good, lo_color.data(), &none, &none, out.data(), P)) return fail("a good call is refused");
  if (us::params_from_abi(nullptr, lo_color.data(), &none, &none, out.data(), P) == nullptr) return fail("null ArtUpsampleParams");
  if (!refused(good, nullptr, &none, &none, out.data(), "null lo_color3f or out3f") || !refused(good, lo_color.data(), &none, &none, nullptr, "null lo_color3f or out3f")) return fail("null planes");
  if (!refused(good, lo_color.data(), nullptr, &none, out.data(), "null ArtUpsampleGuides") || !refused(good, lo_color.data(), &none, nullptr, out.data(), "null ArtUpsampleGuides")) return fail("null guides");
  ArtUpsampleParams b = good; b.width = 0;
  if (!refused(b, lo_color.data(), &none, &none, out.data(), "width and height")) return fail("width");
  b = good; b.width = 1 << 15; b.height = 1 << 14;
  if (!refused(b, lo_color.data(), &none, &none, out.data(), "2^28")) return fail("size");
  b = good; b.lo_width = 5;
  if (!refused(b, lo_color.data(), &none, &none, out.data(), "lo_width")) return fail("lo_width > width");
  b = good; b.lo_height = 0;
  if (!refused(b, lo_color.data(), &none, &none, out.data(), "lo_height")) return fail("lo_height 0");
  b = good; b.footprint = 3;
  if (!refused(b, lo_color.data(), &none, &none, out.data(), "footprint")) return fail("footprint");
  b = good; b.normal_log2 = 11;
  if (!refused(b, lo_color.data(), &none, &none, out.data(), "normal_log2")) return fail("normal_log2");
  b = good; b.scale = INFINITY;
  if (!refused(b, lo_color.data(), &none, &none, out.data(), "scale")) return fail("scale");
  b = good; b.sigma_depth = NAN;
  if (!refused(b, lo_color.data(), &none, &none, out.data(), "sigma_depth")) return fail("sigma_depth");
  b = good; b.jitter[0] = 0.5f;
  if (!refused(b, lo_color.data(), &none, &none, out.data(), "jitter")) return fail("jitter 0.5");
  b = good; b.jitter[1] = NAN;
  if (!refused(b, lo_color.data(), &none, &none, out.data(), "jitter")) return fail("jitter NaN");
  ArtUpsampleGuides one = none; one.depth = plane.data();
  if (!refused(good, lo_color.data(), &one, &none, out.data(), "depth is given on one side only") || !refused(good, lo_color.data(), &none, &one, out.data(), "depth is given on one side only")) return fail("one side");
  b = good; b.demodulate = 1;
  if (!refused(b, lo_color.data(), &none, &none, out.data(), "demodulate")) return fail("demodulate without albedo");
  if (!us::overlap_refusal(P, lo_color.data(), &none, &none, lo_color.data() + 5, nullptr)) return fail("out over lo_color");
  if (!us::overlap_refusal(P, lo_color.data(), &none, &none, out.data(), out.data() + 23)) return fail("fallback over out");
  if (!us::overlap_refusal(P, lo_color.data(), &one, &one, out.data(), plane.data())) return fail("fallback over a guide");
  if (us::overlap_refusal(P, lo_color.data(), &one, &one, out.data(), fb.data())) return fail("no overlap is refused");
  // by hand: 4 x 2 from 2 x 1, no guides, footprint 2: sx = 0.5, u = -0.25, 0.25, 0.75, 1.25: hi pixel 0 has both taps clamped to lo
  // pixel 0; pixel 1 is 0.75 of lo 0 and 0.25 of lo 1; pixel 2 is 0.25 and 0.75; pixel 3 clamps to lo pixel 1.  Both rows are the same.
  run(P, lo_color.data(), none, none, out.data(), fb.data());
  const float want[4] = {1.0f, 1.5f, 2.5f, 3.0f};
  for (int y = 0; y < 2; ++y)
    for (int x = 0; x < 4; ++x) {
      const float* o = &out[3 * (4 * y + x)];
      if (o[0] != want[x] || o[1] != 2.0f * want[x] || o[2] != 4.0f * want[x] || fb[4 * y + x] != 0) return fail("bilinear by hand");
    }
  // a lo pixel without a finite colour is no tap: hi pixels 1 .. 3 take the other's colour, pixel 0 (both taps clamped to the bad one) is
  // black with fallback 2; both bad: every pixel is
  lo_color[1] = NAN;
  run(P, lo_color.data(), none, none, out.data(), fb.data());
  for (int k = 0; k < 8; ++k) if (out[3 * k] != (k % 4 ? 3.0f : 0.0f) || fb[k] != (k % 4 ? 0 : 2)) return fail("a bad lo pixel");
  lo_color[3] = INFINITY;
  run(P, lo_color.data(), none, none, out.data(), fb.data());
  for (int k = 0; k < 8; ++k) if (out[3 * k] != 0.0f || out[3 * k + 2] != 0.0f || fb[k] != 2) return fail("no finite lo pixel");
  // ids: lo pixels 5 and 6; hi ids 5 5 6 6 / 5 9 6 6: each hi pixel takes only its own id's colour; the 9 has no tap and falls back to bilinear
  lo_color = {1.0f, 2.0f, 4.0f, 3.0f, 6.0f, 12.0f};
  const int32_t lo_id[2] = {5, 6}, hi_id[8] = {5, 5, 6, 6, 5, 9, 6, 6};
  ArtUpsampleGuides gl = none, gh = none; gl.id = lo_id; gh.id = hi_id;
  if (us::params_from_abi(&good, lo_color.data(), &gl, &gh, out.data(), P)) return fail("ids are refused");
  run(P, lo_color.data(), gl, gh, out.data(), fb.data());
  const float want_id[8] = {1.0f, 1.0f, 3.0f, 3.0f, 1.0f, 1.5f, 3.0f, 3.0f};
  for (int k = 0; k < 8; ++k) if (out[3 * k] != want_id[k] || fb[k] != (k == 5 ? 1 : 0)) return fail("ids by hand");
  std::printf("upsample_host: ok\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 1) return self_check();
  if (argc != 4 || std::strcmp(argv[1], "run")) return fail("usage: upsample_host [run IN OUT]");
  FILE* f = std::fopen(argv[2], "rb");
  if (!f) return fail("cannot open IN");
  FILE* o = std::fopen(argv[3], "wb");
  if (!o) return fail("cannot open OUT");
  for (;;) {
    ArtUpsampleParams p;
    static_assert(sizeof p == 44, "ArtUpsampleParams is 11 words");
    int32_t given = 0;
    const size_t got = std::fread(&p, 1, sizeof p, f);
    if (got == 0) break;
    if (got != sizeof p || std::fread(&given, 4, 1, f) != 1) return fail("short IN (params)");
    if (p.width < 1 || p.height < 1 || p.lo_width < 1 || p.lo_height < 1 || (long long)p.width * p.height > (1ll << 24) || (long long)p.lo_width * p.lo_height > (1ll << 24)) return fail("bad size");
    const size_t N = (size_t)p.width * (size_t)p.height, NL = (size_t)p.lo_width * (size_t)p.lo_height;
    std::vector<float> lo_color(3 * NL), out(3 * N);
    std::vector<uint8_t> fb(N);
    if (std::fread(lo_color.data(), 4, 3 * NL, f) != 3 * NL) return fail("short IN (lo_color)");
    std::vector<float> pl[2][3];
    std::vector<int32_t> id[2];
    for (int k = 0; k < 4; ++k) {
      if (!(given & (1 << k))) continue;
      for (int side = 0; side < 2; ++side) {
        const size_t n = (side ? N : NL) * (k < 2 ? 3 : 1);
        if (k < 3) { pl[side][k].resize(n); if (std::fread(pl[side][k].data(), 4, n, f) != n) return fail("short IN (a guide)"); }
        else { id[side].resize(n); if (std::fread(id[side].data(), 4, n, f) != n) return fail("short IN (id)"); }
      }
    }
    ArtUpsampleGuides g[2];
    for (int side = 0; side < 2; ++side) {
      g[side].albedo3f = (given & 1) ? pl[side][0].data() : nullptr; g[side].normal3f = (given & 2) ? pl[side][1].data() : nullptr;
      g[side].depth = (given & 4) ? pl[side][2].data() : nullptr; g[side].id = (given & 8) ? id[side].data() : nullptr;
    }
    us::Params P;
    if (const char* why = us::params_from_abi(&p, lo_color.data(), &g[0], &g[1], out.data(), P)) return fail(why);
    if (const char* why = us::overlap_refusal(P, lo_color.data(), &g[0], &g[1], out.data(), fb.data())) return fail(why);
    run(P, lo_color.data(), g[0], g[1], out.data(), fb.data());
    if (std::fwrite(out.data(), 4, 3 * N, o) != 3 * N || std::fwrite(fb.data(), 1, N, o) != N) return fail("short OUT");
  }
  std::fclose(f);
  if (std::fclose(o)) return fail("cannot close OUT");
  return 0;
}
