// TEST-ONLY: the text of art_temporal_upsample_device (csrc/art_temporal_upsample.h) compiled by g++ as a stand-alone program.
//   temporal_upsample_host              its own checks (the refusals of params_from_abi and overlap_refusal, a few values by hand); prints
//                                       "temporal_upsample_host: ok"
//   temporal_upsample_host run IN OUT   IN:  one call after the other until the file ends, each: ArtTemporalUpsampleParams (53 words; prev's
//                                            size is the history's), given (int32: bit 0 normal, 1 depth, 2 id, 3 motion, 4 hist_in),
//                                            lo_color (3 floats per lo pixel), lo_moments (2), then for every guide given, in that order,
//                                            its lo plane and its hi plane, then the hi motion plane, then hist_in (row-major)
//                                       OUT: per call hist_out (12 words per hi pixel), out3f (3), variance_out (1), length_out (1), then
//                                            fallback1b (1 byte per hi pixel)
// tests/test_temporal_upsample_reference_host.py holds OUT to tests/temporal_upsample_ref.py bit for bit.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "art_temporal_upsample.h"

using namespace art;

static int fail(const char* what) { std::fprintf(stderr, "temporal_upsample_host: %s\n", what); return 1; }

// the two kernels of art_temporal_upsample.hip over arrays: pack every lo pixel, then every hi pixel
static void run(const tu::Params& P, const float* lo_color, const float* lo_moments, const ArtTemporalUpsampleGuides& lo, const ArtTemporalUpsampleGuides& hi,
                const tu::Rec4* hist_in, tu::Rec4* hist_out, float* out, float* variance, float* length, uint8_t* fallback) {
  const size_t NL = (size_t)P.LW * (size_t)P.LH, N = (size_t)P.T.cur.W * (size_t)P.T.cur.H;
  std::vector<tu::Rec4> a(NL), b(NL), c(NL);
  for (size_t q = 0; q < NL; ++q) tu::pack_lo(P, lo_color, lo_moments, lo.normal3f, lo.depth, lo.id, q, a[q], b[q], c[q]);
  for (int y = 0; y < P.T.cur.H; ++y)
    for (int x = 0; x < P.T.cur.W; ++x) {
      const size_t p = (size_t)y * (size_t)P.T.cur.W + (size_t)x;
      const tu::Out o = hi.motion3f ? tu::temporal_upsample_pixel<true>(P, a.data(), b.data(), c.data(), hi.normal3f, hi.depth, hi.id, hi.motion3f, hist_in, x, y)
                                    : tu::temporal_upsample_pixel<false>(P, a.data(), b.data(), c.data(), hi.normal3f, hi.depth, hi.id, nullptr, hist_in, x, y);
      hist_out[p] = o.h0; hist_out[N + p] = o.h1; hist_out[2 * N + p] = o.h2;
      out[3 * p] = o.h0.x; out[3 * p + 1] = o.h0.y; out[3 * p + 2] = o.h0.z;
      variance[p] = o.variance; length[p] = o.h0.w; fallback[p] = o.fallback;
    }
}

static ArtTemporalUpsampleParams good_params(int w, int h, int lw, int lh) {
  ArtTemporalUpsampleParams p;
  std::memset(&p, 0, sizeof p);
  for (int k = 0; k < 4; ++k) p.t.cur.cam_matrix[5 * k] = 1.0f;
  p.t.cur.width = w; p.t.cur.height = h;
  p.t.prev = p.t.cur;
  p.t.n_colours = 1; p.t.max_history = 8; p.t.scale = 1.0f; p.t.depth_tol = 0.05f; p.t.normal_min = 0.9f;
  p.lo_width = lw; p.lo_height = lh; p.radius = 1.0f; p.min_confidence = 0.5f;
  return p;
}

static bool refused(const ArtTemporalUpsampleParams& p, const void* c, const void* m, const ArtTemporalUpsampleGuides* lo, const ArtTemporalUpsampleGuides* hi,
                    const void* hin, const void* hout, const char* text) {
  tu::Params P;
  const char* why = tu::params_from_abi(&p, c, m, lo, hi, hin, hout, P);
  return why && std::strstr(why, text);
}

static int self_check() {
  const ArtTemporalUpsampleParams good = good_params(4, 2, 2, 1);
  std::vector<float> lc = {1.0f, 2.0f, 4.0f, 3.0f, 6.0f, 12.0f}, lm = {1.0f, 2.0f, 3.0f, 10.0f}, out(24), var(8), len(8), plane(24, 0.5f);
  std::vector<tu::Rec4> hout(24), hin(24);
  std::vector<uint8_t> fb(8);
  const ArtTemporalUpsampleGuides none = {nullptr, nullptr, nullptr, nullptr};
  tu::Params P;
  if (tu::params_from_abi(&good, lc.data(), lm.data(), &none, &none, nullptr, hout.data(), P)) return fail("a good call is refused");
  if (!tu::params_from_abi(nullptr, lc.data(), lm.data(), &none, &none, nullptr, hout.data(), P)) return fail("null params");
  if (!refused(good, nullptr, lm.data(), &none, &none, nullptr, hout.data(), "null lo_color3f") || !refused(good, lc.data(), nullptr, &none, &none, nullptr, hout.data(), "null lo_color3f") ||
      !refused(good, lc.data(), lm.data(), &none, &none, nullptr, nullptr, "null lo_color3f"))
    return fail("null planes");
  if (!refused(good, lc.data(), lm.data(), nullptr, &none, nullptr, hout.data(), "null ArtTemporalUpsampleGuides") ||
      !refused(good, lc.data(), lm.data(), &none, nullptr, nullptr, hout.data(), "null ArtTemporalUpsampleGuides"))
    return fail("null guides");
  ArtTemporalUpsampleGuides one = none; one.depth = plane.data();
  if (!refused(good, lc.data(), lm.data(), &one, &none, nullptr, hout.data(), "depth is given on one side only") ||
      !refused(good, lc.data(), lm.data(), &none, &one, nullptr, hout.data(), "depth is given on one side only"))
    return fail("one side");
  ArtTemporalUpsampleGuides mo = none; mo.motion3f = plane.data();
  if (!refused(good, lc.data(), lm.data(), &mo, &none, nullptr, hout.data(), "lo motion3f")) return fail("lo motion");
  if (tu::params_from_abi(&good, lc.data(), lm.data(), &none, &mo, nullptr, hout.data(), P)) return fail("hi motion is refused");
  ArtTemporalUpsampleParams b = good; b.t.cur.width = 0;
  if (!refused(b, lc.data(), lm.data(), &none, &none, nullptr, hout.data(), "cur: width and height")) return fail("width");
  b = good; b.t.n_colours = 0;
  if (!refused(b, lc.data(), lm.data(), &none, &none, nullptr, hout.data(), "n_colours")) return fail("n_colours");
  b = good; b.t.cur.cam_matrix[3] = 1.0f;
  if (!refused(b, lc.data(), lm.data(), &none, &none, nullptr, hout.data(), "camera is refused")) return fail("camera");
  if (!refused(good, lc.data(), lm.data(), &none, &none, hout.data() + 3, hout.data(), "hist_in and hist_out overlap")) return fail("histories");
  b = good; b.lo_width = 5;
  if (!refused(b, lc.data(), lm.data(), &none, &none, nullptr, hout.data(), "lo_width")) return fail("lo_width > width");
  b = good; b.lo_height = 0;
  if (!refused(b, lc.data(), lm.data(), &none, &none, nullptr, hout.data(), "lo_height")) return fail("lo_height 0");
  b = good; b.jitter[0] = 0.5f;
  if (!refused(b, lc.data(), lm.data(), &none, &none, nullptr, hout.data(), "jitter")) return fail("jitter 0.5");
  b = good; b.jitter[1] = NAN;
  if (!refused(b, lc.data(), lm.data(), &none, &none, nullptr, hout.data(), "jitter")) return fail("jitter NaN");
  for (float r : {0.0f, -1.0f, 2.5f, NAN, INFINITY}) {
    b = good; b.radius = r;
    if (!refused(b, lc.data(), lm.data(), &none, &none, nullptr, hout.data(), "radius")) return fail("radius");
  }
  b = good; b.radius = 2.0f;              // the bound itself: min(4 / 2, 2 / 1)
  if (tu::params_from_abi(&b, lc.data(), lm.data(), &none, &none, nullptr, hout.data(), P)) return fail("radius at the bound is refused");
  for (float m : {0.0f, -0.5f, 1.5f, NAN}) {
    b = good; b.min_confidence = m;
    if (!refused(b, lc.data(), lm.data(), &none, &none, nullptr, hout.data(), "min_confidence")) return fail("min_confidence");
  }
  if (tu::params_from_abi(&good, lc.data(), lm.data(), &none, &none, nullptr, hout.data(), P)) return fail("a good call is refused");
  if (!tu::overlap_refusal(P, lc.data(), lm.data(), &none, &none, nullptr, hout.data(), lc.data() + 5, nullptr, nullptr, nullptr)) return fail("out over lo_color");
  if (!tu::overlap_refusal(P, lc.data(), lm.data(), &none, &none, nullptr, hout.data(), out.data(), nullptr, nullptr, (const uint8_t*)out.data() + 95)) return fail("fallback over out");
  if (!tu::overlap_refusal(P, lc.data(), lm.data(), &one, &one, nullptr, hout.data(), out.data(), plane.data(), nullptr, nullptr)) return fail("variance over a guide");
  if (!tu::overlap_refusal(P, lc.data(), lm.data(), &none, &none, nullptr, hout.data(), out.data(), var.data(), hout.data() + 23, nullptr)) return fail("length over hist_out");
  if (tu::overlap_refusal(P, lc.data(), lm.data(), &one, &one, nullptr, hout.data(), out.data(), var.data(), len.data(), fb.data())) return fail("no overlap is refused");
  // by hand: 4 x 2 from 2 x 1, no guides, no history, jitter 0, radius 1: sx = 0.5, u = -0.25, 0.25, 0.75, 1.25, sy = 0.5, v = -0.25, 0.25:
  // hi pixel 0 keeps lo pixel 0 alone (its left tap is outside), pixel 1 is 0.75 of lo 0 and 0.25 of lo 1, pixel 2 the reverse, pixel 3
  // lo 1 alone; in y one tap row is inside.  Every sample lies 0.5 hi pixels off in each axis: K = 0.25 per tap pair's weight share.
  run(P, lc.data(), lm.data(), none, none, nullptr, hout.data(), out.data(), var.data(), len.data(), fb.data());
  const float want[4] = {1.0f, 1.5f, 2.5f, 3.0f};
  for (int y = 0; y < 2; ++y)
    for (int x = 0; x < 4; ++x) {
      const float* o = &out[3 * (4 * y + x)];
      if (o[0] != want[x] || o[1] != 2.0f * want[x] || o[2] != 4.0f * want[x] || fb[4 * y + x] != 0) return fail("bilinear by hand");
      if (len[4 * y + x] != 0.5f) return fail("the length of a pixel without history is n_cur * max(kappa, min_confidence)");      // kappa = 0.25 < 0.5
      if (var[4 * y + x] != INFINITY) return fail("variance below two colours");
    }
  // the second frame on that history, cameras at rest: n_eff = 0.25, n = 0.25 + 0.5, a = 1 / 3
  hin = hout;
  ArtTemporalUpsampleParams second = good;
  if (tu::params_from_abi(&second, lc.data(), lm.data(), &none, &none, hin.data(), hout.data(), P)) return fail("the second frame is refused");
  run(P, lc.data(), lm.data(), none, none, hin.data(), hout.data(), out.data(), var.data(), len.data(), fb.data());
  for (int k = 0; k < 8; ++k) if (len[k] != 0.75f || fb[k] != 0) return fail("the second frame's length");
  // a lo pixel without a finite colour is no tap; both bad: every pixel is zero with fallback 2 and length 0
  lc[1] = NAN; lc[3] = INFINITY;
  if (tu::params_from_abi(&good, lc.data(), lm.data(), &none, &none, nullptr, hout.data(), P)) return fail("a good call is refused");
  run(P, lc.data(), lm.data(), none, none, nullptr, hout.data(), out.data(), var.data(), len.data(), fb.data());
  for (int k = 0; k < 8; ++k) if (out[3 * k] != 0.0f || out[3 * k + 2] != 0.0f || len[k] != 0.0f || fb[k] != 2) return fail("no finite lo pixel");
  // ids: lo pixels 5 and 6; hi ids 5 5 6 6 / 5 9 6 6: each hi pixel takes only its own id's colour; the 9 has no tap and is the unguided mean
  lc = {1.0f, 2.0f, 4.0f, 3.0f, 6.0f, 12.0f};
  const int32_t lo_id[2] = {5, 6}, hi_id[8] = {5, 5, 6, 6, 5, 9, 6, 6};
  ArtTemporalUpsampleGuides gl = none, gh = none; gl.id = lo_id; gh.id = hi_id;
  if (tu::params_from_abi(&good, lc.data(), lm.data(), &gl, &gh, nullptr, hout.data(), P)) return fail("ids are refused");
  run(P, lc.data(), lm.data(), gl, gh, nullptr, hout.data(), out.data(), var.data(), len.data(), fb.data());
  const float want_id[8] = {1.0f, 1.0f, 3.0f, 3.0f, 1.0f, 1.5f, 3.0f, 3.0f};
  for (int k = 0; k < 8; ++k) if (out[3 * k] != want_id[k] || fb[k] != (k == 5 ? 1 : 0)) return fail("ids by hand");
  std::printf("temporal_upsample_host: ok\n");
  return 0;
}

template <class T>
static bool read_plane(FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return std::fread(v.data(), sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc == 1) return self_check();
  if (argc != 4 || std::strcmp(argv[1], "run")) return fail("usage: temporal_upsample_host [run IN OUT]");
  FILE* f = std::fopen(argv[2], "rb");
  if (!f) return fail("cannot open IN");
  FILE* o = std::fopen(argv[3], "wb");
  if (!o) return fail("cannot open OUT");
  for (;;) {
    ArtTemporalUpsampleParams p;
    static_assert(sizeof p == 212, "ArtTemporalUpsampleParams is 53 words");
    int32_t given = 0;
    const size_t got = std::fread(&p, 1, sizeof p, f);
    if (got == 0) break;
    if (got != sizeof p || std::fread(&given, 4, 1, f) != 1) return fail("short IN (params)");
    const bool has_hist = (given & 16) != 0;
    const long long lim = 1ll << 24;
    if (p.t.cur.width < 1 || p.t.cur.height < 1 || p.lo_width < 1 || p.lo_height < 1 || (long long)p.t.cur.width * p.t.cur.height > lim || (long long)p.lo_width * p.lo_height > lim)
      return fail("bad size");
    if (has_hist && (p.t.prev.width < 1 || p.t.prev.height < 1 || (long long)p.t.prev.width * p.t.prev.height > lim)) return fail("bad size (prev)");
    const size_t N = (size_t)p.t.cur.width * (size_t)p.t.cur.height, NL = (size_t)p.lo_width * (size_t)p.lo_height;
    const size_t NP = has_hist ? (size_t)p.t.prev.width * (size_t)p.t.prev.height : 0;
    std::vector<float> lc, lm, pl[2][2], motion, out(3 * N), var(N), len(N);
    std::vector<int32_t> id[2];
    std::vector<tu::Rec4> hin, hout(3 * N);
    std::vector<uint8_t> fb(N);
    if (!read_plane(f, lc, 3 * NL) || !read_plane(f, lm, 2 * NL)) return fail("short IN (lo_color, lo_moments)");
    for (int k = 0; k < 3; ++k) {
      if (!(given & (1 << k))) continue;
      for (int side = 0; side < 2; ++side) {
        const size_t n = (side ? N : NL) * (k == 0 ? 3 : 1);
        if (!(k < 2 ? read_plane(f, pl[side][k], n) : read_plane(f, id[side], n))) return fail("short IN (a guide)");
      }
    }
    if ((given & 8) && !read_plane(f, motion, 3 * N)) return fail("short IN (motion)");
    if (has_hist && !read_plane(f, hin, 3 * NP)) return fail("short IN (hist_in)");
    ArtTemporalUpsampleGuides g[2];
    for (int side = 0; side < 2; ++side) {
      g[side].normal3f = (given & 1) ? pl[side][0].data() : nullptr; g[side].depth = (given & 2) ? pl[side][1].data() : nullptr;
      g[side].id = (given & 4) ? id[side].data() : nullptr; g[side].motion3f = nullptr;
    }
    if (given & 8) g[1].motion3f = motion.data();
    const tu::Rec4* hist_in = has_hist ? hin.data() : nullptr;
    tu::Params P;
    if (const char* why = tu::params_from_abi(&p, lc.data(), lm.data(), &g[0], &g[1], hist_in, hout.data(), P)) return fail(why);
    if (const char* why = tu::overlap_refusal(P, lc.data(), lm.data(), &g[0], &g[1], hist_in, hout.data(), out.data(), var.data(), len.data(), fb.data())) return fail(why);
    run(P, lc.data(), lm.data(), g[0], g[1], hist_in, hout.data(), out.data(), var.data(), len.data(), fb.data());
    if (std::fwrite(hout.data(), 16, 3 * N, o) != 3 * N || std::fwrite(out.data(), 4, 3 * N, o) != 3 * N || std::fwrite(var.data(), 4, N, o) != N ||
        std::fwrite(len.data(), 4, N, o) != N || std::fwrite(fb.data(), 1, N, o) != N)
      return fail("short OUT");
  }
  std::fclose(f);
  if (std::fclose(o)) return fail("cannot close OUT");
  return 0;
}
