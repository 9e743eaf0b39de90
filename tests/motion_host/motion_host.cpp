// TEST-ONLY: the motion plane of art_render_aovs_motion_device and art_temporal_motion_device on host arrays, through the product's own
// per-hit and per-pixel text (csrc/art_motion.h, csrc/art_temporal.h) compiled by g++.  Pointers are host memory.  With
// -DMOTION_HOST_MAIN the file is a program that runs both over inputs of its own and checks what can be checked without a reference
// (the sanitizer build's target).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "art_hip.h"
#include "../../ada-ray-tracer_amd/csrc/art_motion.h"
#include "../../ada-ray-tracer_amd/csrc/art_temporal.h"

using namespace art;

// n pixels with K rays each, ray s of pixel l at s * n + l (the slots of a slice): key, t, u, v per ray, dirs3 3 floats per ray.
// inst: DevInstance records (32 words each), or nullptr for a flat scene.
extern "C" int mh_plane(int32_t K, int32_t n, const uint32_t* key, const float* t, const float* u, const float* v, const float* dirs3, const float* cam,
                        const int32_t* idx, const float* cur, const float* prev, const void* inst, const float* prev_m, int32_t inst_shift, float* out3) {
  if ((K != 1 && K != 4) || n < 0) return 1;
  mo::Source S;
  S.idx = idx; S.cur = cur; S.prev = prev; S.inst = (const DevInstance*)inst; S.prev_m = prev_m; S.inst_shift = inst_shift;
  for (int l = 0; l < n; ++l) {
    mo::V3 d[4] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int s = 0; s < K; ++s) {
      const size_t i = (size_t)s * n + l;
      d[s] = mo::hit_delta(S, cam, key[i], t[i], u[i], v[i], dirs3[3 * i], dirs3[3 * i + 1], dirs3[3 * i + 2]);
    }
    if (K == 4) { out3[3 * l] = mo::mean4(d[0].x, d[1].x, d[2].x, d[3].x); out3[3 * l + 1] = mo::mean4(d[0].y, d[1].y, d[2].y, d[3].y); out3[3 * l + 2] = mo::mean4(d[0].z, d[1].z, d[2].z, d[3].z); }
    else { out3[3 * l] = d[0].x; out3[3 * l + 1] = d[0].y; out3[3 * l + 2] = d[0].z; }
  }
  return 0;
}

extern "C" int mh_temporal_motion(const ArtTemporalParams* p, const float* color3f, const float* moments2f, const float* normal3f, const float* depth,
                                  const int32_t* id, const float* motion3f, const void* hist_in, void* hist_out, float* out3f, float* variance_out, float* length_out) {
  tp::Params P;
  if (tp::params_from_abi(p, color3f, moments2f, normal3f, depth, id, hist_in, hist_out, P, motion3f)) return 1;      // (the library's own derivation and refusals)
  const size_t N = (size_t)P.cur.W * (size_t)P.cur.H;
  tp::Rec4* ho = (tp::Rec4*)hist_out;
  for (int y = 0; y < P.cur.H; ++y)
    for (int x = 0; x < P.cur.W; ++x) {
      const size_t q = (size_t)y * P.cur.W + x;
      const tp::Out o = motion3f ? tp::temporal_pixel<true>(P, color3f, moments2f, normal3f, depth, id, (const tp::Rec4*)hist_in, x, y, motion3f)
                                 : tp::temporal_pixel(P, color3f, moments2f, normal3f, depth, id, (const tp::Rec4*)hist_in, x, y);
      ho[q] = o.h0; ho[N + q] = o.h1; ho[2 * N + q] = o.h2;
      if (out3f) { out3f[3 * q] = o.h0.x; out3f[3 * q + 1] = o.h0.y; out3f[3 * q + 2] = o.h0.z; }
      if (variance_out) variance_out[q] = o.variance;
      if (length_out) length_out[q] = o.h0.w;
    }
  return 0;
}

#ifdef MOTION_HOST_MAIN
static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }
static float uni(uint32_t& s) { return (float)lcg(s) * (1.0f / 16777216.0f); }

int main() {
  uint32_t seed = 99u;
  int bad = 0;
  // a flat mesh of 40 triangles over 60 vertices, the odd ones moved; every class of key; K = 4 and 1
  const int nv = 60, nt = 40, n = 77;
  std::vector<float> cur(3 * nv), prev(3 * nv);
  std::vector<int32_t> idx(3 * nt);
  for (int k = 0; k < 3 * nv; ++k) { cur[k] = 4.0f * uni(seed) - 2.0f; prev[k] = ((k / 3) & 1) ? cur[k] + 0.25f * uni(seed) : cur[k]; }
  for (int k = 0; k < 3 * nt; ++k) idx[k] = (int32_t)(lcg(seed) % nv);
  idx[0] = 0; idx[1] = 2; idx[2] = 4;                                         // an unmoved triple
  const float cam[3] = {0.1f, 0.2f, 0.3f};
  for (int K : {4, 1}) {
    std::vector<uint32_t> key((size_t)K * n);
    std::vector<float> t((size_t)K * n), u((size_t)K * n), v((size_t)K * n), d(3 * (size_t)K * n), out(3 * n);
    for (size_t i = 0; i < key.size(); ++i) {
      const uint32_t c = lcg(seed) % 6;
      key[i] = (c == 5) ? KEY_MISS : (c << 28) | (c == 4 ? lcg(seed) % nt : lcg(seed) % 3);
      if (i % 7 == 0) key[i] = KEY_TRI;                                       // triangle 0
      t[i] = 1.0f + uni(seed); u[i] = 0.5f * uni(seed); v[i] = 0.5f * uni(seed);
      for (int k = 0; k < 3; ++k) d[3 * i + k] = uni(seed) - 0.5f;
    }
    if (mh_plane(K, n, key.data(), t.data(), u.data(), v.data(), d.data(), cam, idx.data(), cur.data(), prev.data(), nullptr, nullptr, 0, out.data())) { std::puts("mh_plane refused"); return 1; }
    for (int l = 0; l < n; ++l) {
      bool moved = false;
      for (int s = 0; s < K; ++s) { const uint32_t k = key[(size_t)s * n + l]; if (k != KEY_MISS && (k & ~KEY_INDEX_MASK) == KEY_TRI && (k & KEY_INDEX_MASK) != 0) moved = true; }
      for (int k = 0; k < 3; ++k) {
        const float x = out[3 * l + k];
        if (!std::isfinite(x) || std::fabs(x) > 0.25f) { std::printf("K = %d pixel %d: component %d is %g\n", K, l, k, x); ++bad; }
        if (!moved && (x != 0.0f || std::signbit(x))) { std::printf("K = %d pixel %d: nothing moved, component %d is %g\n", K, l, k, x); ++bad; }
      }
    }
    // no vertex arrays: all +0
    mh_plane(K, n, key.data(), t.data(), u.data(), v.data(), d.data(), cam, idx.data(), nullptr, nullptr, nullptr, nullptr, 0, out.data());
    for (float x : out) if (x != 0.0f || std::signbit(x)) { std::puts("no vertex arrays, but a delta"); ++bad; break; }
    // instanced: two instances, the second translated since the previous update
    DevInstance inst[2]; std::memset(inst, 0, sizeof inst);
    float pm[24];
    for (int j = 0; j < 2; ++j) {
      for (int r = 0; r < 3; ++r) { inst[j].m[4 * r + r] = 2.0f; inst[j].minv[4 * r + r] = 0.5f; inst[j].m[4 * r + 3] = (float)(j + r); inst[j].minv[4 * r + 3] = -0.5f * (float)(j + r); }
      std::memcpy(pm + 12 * j, inst[j].m, 48);
    }
    pm[12 + 3] -= 0.75f;
    for (size_t i = 0; i < key.size(); ++i) if (key[i] != KEY_MISS && (key[i] & ~KEY_INDEX_MASK) == KEY_TRI) key[i] = KEY_TRI | ((uint32_t)(i & 1) << 6) | (key[i] & 63u);
    mh_plane(K, n, key.data(), t.data(), u.data(), v.data(), d.data(), cam, nullptr, nullptr, nullptr, inst, pm, 6, out.data());
    for (int l = 0; l < n; ++l) {
      if (!(out[3 * l] <= 0.0f && out[3 * l] >= -0.76f) || out[3 * l + 1] != 0.0f || out[3 * l + 2] != 0.0f) { std::printf("K = %d pixel %d: instanced delta (%g, %g, %g)\n", K, l, out[3 * l], out[3 * l + 1], out[3 * l + 2]); ++bad; }
    }
  }
  // the temporal path: cameras at rest, zero motion -> the history grows as without motion; NaN motion -> the pixel starts again
  {
    const int W = 13, H = 9; const size_t N = (size_t)W * H;
    std::vector<float> color(3 * N), mom(2 * N), nrm(3 * N), dep(N), mot(3 * N, 0.0f), out(3 * N), var(N), len(N), h0(12 * N), h1(12 * N);
    std::vector<int32_t> id(N, 1);
    for (size_t k = 0; k < N; ++k) {
      for (int c = 0; c < 3; ++c) { color[3 * k + c] = 4.0f * uni(seed); nrm[3 * k + c] = (c == 2) ? 1.0f : 0.0f; }
      const float l = dn::lum3(color[3 * k], color[3 * k + 1], color[3 * k + 2]);
      mom[2 * k] = l; mom[2 * k + 1] = l * l / 4.0f * (1.0f + uni(seed)); dep[k] = 10.0f;
    }
    ArtTemporalParams p; std::memset(&p, 0, sizeof p);
    p.cur.cam_matrix[0] = p.cur.cam_matrix[5] = p.cur.cam_matrix[10] = p.cur.cam_matrix[15] = 1.0f; p.cur.width = W; p.cur.height = H; p.prev = p.cur;
    p.n_colours = 4; p.max_history = 64; p.scale = 0.25f; p.depth_tol = 0.1f; p.normal_min = 0.9f;
    if (mh_temporal_motion(&p, color.data(), mom.data(), nrm.data(), dep.data(), id.data(), mot.data(), nullptr, h0.data(), out.data(), var.data(), len.data())) { std::puts("first frame refused"); return 1; }
    mot[3 * 5] = NAN;
    if (mh_temporal_motion(&p, color.data(), mom.data(), nrm.data(), dep.data(), id.data(), mot.data(), h0.data(), h1.data(), out.data(), var.data(), len.data())) { std::puts("second frame refused"); return 1; }
    for (size_t k = 0; k < N; ++k) {
      const float want = (k == 5) ? 4.0f : 8.0f;
      if (!(std::fabs(len[k] - want) < 1e-3f)) { std::printf("temporal: pixel %zu has length %g, not %g\n", k, len[k], want); ++bad; }
    }
  }
  std::printf("motion_host: %s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
#endif
