// art_temporal_upsample.h -- the per-pixel text of art_temporal_upsample_device (include/art_hip.h states the arithmetic; this is its one
// definition): the preparation of a lo pixel, the splat of this frame's lo samples into a hi pixel, the gather of the hi history, the
// combination of the two, and the refusals of the call's arguments.  ART_HD functions over plain pointers, no HIP types:
// art_temporal_upsample.hip compiles them for gfx950 and tests/temporal_upsample_host compiles the same text with g++ (the arrangement of
// art_upsample.h with tests/upsample_host), so the kernels and the host build cannot drift apart.  The mapping of an axis is us::map_axis
// (art_upsample.h) and the dot product tp::dot3 (art_temporal.h), called, not retyped; the gather of the history is art_temporal.h's,
// restated here (temporal_pixel is one function, and carving a shared piece out of it would change the existing kernel's code).
//
// Working data (the library's scratch, one entry per LO pixel, row-major, three planes of LW * LH records):
//   a  Rec4 {r, g, b, m1}          c(q) = scale * colour and m1 = S1 / n_cur
//   b  Rec4 {m2, z, id, word}      m2 = S2 / n_cur, the lo depth (0 without a plane), the lo id's int32 as a word (0 without a plane) and,
//                                  as a word, bit 0 = bad in guides, bit 1 = bad in colour
//   c  Rec4 {nx, ny, nz, 0}        the lo normal (read only where normals are given)
// so a tap costs two or three 16-byte loads, and the two divisions of a lo pixel are done once, not once per hi pixel that taps it.
#pragma once
#include "art_temporal.h"
#include "art_upsample.h"

namespace art {
namespace tu {

using dn::Rec4;
using dn::finite_f;

struct Params {
  tp::Params T;                    // the hi cameras, which planes are given, the reprojection rule, n_cur, max_history, scale, depth_tol, normal_min
  int32_t LW, LH;
  float jx, jy, radius, min_confidence;
};

constexpr uint32_t kBadGuides = 1u, kBadColour = 2u;

// preparation of lo pixel q (a linear index)
ART_HD void pack_lo(const Params& P, const float* color, const float* moments, const float* normal, const float* depth, const int32_t* id, size_t q,
                    Rec4& a, Rec4& b, Rec4& c) {
  a.x = P.T.scale * color[3 * q]; a.y = P.T.scale * color[3 * q + 1]; a.z = P.T.scale * color[3 * q + 2];
  a.w = moments[2 * q] / P.T.n_cur; b.x = moments[2 * q + 1] / P.T.n_cur;
  uint32_t flags = (finite_f(a.x) && finite_f(a.y) && finite_f(a.z) && finite_f(a.w) && finite_f(b.x)) ? 0u : kBadColour;
  c.x = c.y = c.z = c.w = 0.0f;
  if (P.T.has_normal) {
    c.x = normal[3 * q]; c.y = normal[3 * q + 1]; c.z = normal[3 * q + 2];
    if (!(finite_f(c.x) && finite_f(c.y) && finite_f(c.z))) flags |= kBadGuides;
  }
  b.y = 0.0f;
  if (P.T.has_depth) {
    b.y = depth[q];
    if (!finite_f(b.y)) flags |= kBadGuides;
  }
  b.z = __builtin_bit_cast(float, P.T.has_id ? id[q] : (int32_t)0);
  b.w = __builtin_bit_cast(float, flags);
}

struct Out { Rec4 h0, h1, h2; float variance; uint8_t fallback; };

// hi pixel (x, y): its three history records, the variance of its mean luminance and its fallback byte.  MOTION: the hi motion plane is
// given (P.T comes from tp::params_from_abi with that plane named) and the world point of the history look-up is taken back by the
// pixel's delta, as in tp::temporal_pixel<true>.
template <bool MOTION>
ART_HD Out temporal_upsample_pixel(const Params& P, const Rec4* lo_a, const Rec4* lo_b, const Rec4* lo_c, const float* normal, const float* depth,
                                   const int32_t* id, const float* motion, const Rec4* hist, int x, int y) {
  const tp::Params& T = P.T;
  const size_t p = (size_t)y * (size_t)T.cur.W + (size_t)x;
  const float z = T.has_depth ? depth[p] : 0.0f;
  const int32_t pid = T.has_id ? id[p] : 0;
  float nx = 0.0f, ny = 0.0f, nz = 0.0f;
  if (T.has_normal) { nx = normal[3 * p]; ny = normal[3 * p + 1]; nz = normal[3 * p + 2]; }
  bool bad = false;                                                // a given hi guide that is not finite: no tap counts
  if (T.has_depth && !finite_f(z)) bad = true;
  if (T.has_normal && !(finite_f(nx) && finite_f(ny) && finite_f(nz))) bad = true;
  const bool miss = T.has_depth && !(z > 0.0f);

  // ---- A. this frame: the 2 x 2 lo samples around the pixel, under the narrow tent (k), the bilinear weight (h, counting taps) and the
  // bilinear weight again over every tap with a finite colour (the unguided mean)
  int i0, j0; float fx, fy, sx, sy;
  us::map_axis(x, T.cur.W, P.LW, P.jx, i0, fx, sx);
  us::map_axis(y, T.cur.H, P.LH, P.jy, j0, fy, sy);
  float K = 0.0f, kr = 0.0f, kg = 0.0f, kb = 0.0f, km1 = 0.0f, km2 = 0.0f;
  float Hs = 0.0f, er = 0.0f, eg = 0.0f, eb = 0.0f, em1 = 0.0f, em2 = 0.0f;
  float Ua = 0.0f, ur = 0.0f, ug = 0.0f, ub = 0.0f, um1 = 0.0f, um2 = 0.0f;
  for (int t = 0; t < 4; ++t) {
    const int a = t & 1, b = t >> 1;
    const int qx = i0 + a, qy = j0 + b;
    if (qx < 0 || qx >= P.LW || qy < 0 || qy >= P.LH) continue;
    const size_t q = (size_t)qy * (size_t)P.LW + (size_t)qx;
    const Rec4 B = lo_b[q];
    const uint32_t flags = __builtin_bit_cast(uint32_t, B.w);
    if (flags & kBadColour) continue;
    const Rec4 A = lo_a[q];
    const float h = (a ? fx : 1.0f - fx) * (b ? fy : 1.0f - fy);
    if (h > 0.0f) { Ua += h; ur += h * A.x; ug += h * A.y; ub += h * A.z; um1 += h * A.w; um2 += h * B.x; }
    if (bad || (flags & kBadGuides)) continue;
    if (T.has_id && __builtin_bit_cast(int32_t, B.z) != pid) continue;
    if (miss) {
      if (B.y > 0.0f) continue;                                    // a hi miss counts lo misses only
    } else {
      if (T.has_normal) {
        const Rec4 Cn = lo_c[q];
        if (!(tp::dot3(nx, ny, nz, Cn.x, Cn.y, Cn.z) >= T.normal_min)) continue;
      }
      if (T.has_depth && !(fabsf(B.y - z) <= T.depth_tol * z)) continue;
    }
    if (h > 0.0f) { Hs += h; er += h * A.x; eg += h * A.y; eb += h * A.z; em1 += h * A.w; em2 += h * B.x; }
    const float dx = ((float)a - fx) / sx, dy = ((float)b - fy) / sy;
    const float k = amax(0.0f, 1.0f - fabsf(dx) / P.radius) * amax(0.0f, 1.0f - fabsf(dy) / P.radius);
    if (k > 0.0f) { K += k; kr += k * A.x; kg += k * A.y; kb += k * A.z; km1 += k * A.w; km2 += k * B.x; }
  }
  const float kappa = (K < 1.0f) ? K : 1.0f;

  // ---- B. the history: art_temporal_device's steps 2 to 4 on the hi guides and the hi cameras (art_temporal.h's text, restated)
  bool own = !T.has_hist;
  if (T.has_depth && !(z > 0.0f && finite_f(z))) own = true;
  if (T.has_normal && !(finite_f(nx) && finite_f(ny) && finite_f(nz))) own = true;
  float hr = 0.0f, hg = 0.0f, hb = 0.0f, hn = 0.0f, hm1 = 0.0f, hm2 = 0.0f, wsum = 0.0f;
  if (!own) {
    float gfx = (float)x + 0.5f, gfy = (float)y + 0.5f, e = z;
    bool ok = true;
    if (T.reproject) {
      const float rx = ((float)x + 0.5f) - ((float)T.cur.W / 2.0f), ry = ((float)y + 0.5f) - ((float)T.cur.H / 2.0f), rz = T.cur.cam_z;
      const float li = 1.0f / sqrtf(tp::dot3(rx, ry, rz, rx, ry, rz));
      const float ux = li * rx, uy = li * ry, uz = li * rz;
      const float* M = T.cur.m;
      const float tx = (M[0] * ux + M[1] * uy) + M[2] * uz, ty = (M[3] * ux + M[4] * uy) + M[5] * uz, tz = (M[6] * ux + M[7] * uy) + M[8] * uz;
      const float lj = 1.0f / sqrtf(tp::dot3(tx, ty, tz, tx, ty, tz));
      const float dx = lj * tx, dy = lj * ty, dz = lj * tz;
      float vx, vy, vz;
      if constexpr (MOTION) {
        const float mx = motion[3 * p], my = motion[3 * p + 1], mz = motion[3 * p + 2];
        if (!(finite_f(mx) && finite_f(my) && finite_f(mz))) ok = false;
        vx = ((T.cur.pos[0] + z * dx) + mx) - T.prev.pos[0]; vy = ((T.cur.pos[1] + z * dy) + my) - T.prev.pos[1]; vz = ((T.cur.pos[2] + z * dz) + mz) - T.prev.pos[2];
      } else {
        vx = (T.cur.pos[0] + z * dx) - T.prev.pos[0]; vy = (T.cur.pos[1] + z * dy) - T.prev.pos[1]; vz = (T.cur.pos[2] + z * dz) - T.prev.pos[2];
      }
      e = sqrtf(tp::dot3(vx, vy, vz, vx, vy, vz));
      const float* I = T.prev.minv;
      const float qx = (I[0] * vx + I[1] * vy) + I[2] * vz, qy = (I[3] * vx + I[4] * vy) + I[5] * vz, qz = (I[6] * vx + I[7] * vy) + I[8] * vz;
      if (!(qz * T.prev.cam_z > 0.0f)) ok = false;               // behind the previous camera, or NaN
      const float k = T.prev.cam_z / qz;
      gfx = qx * k + (float)T.prev.W / 2.0f; gfy = qy * k + (float)T.prev.H / 2.0f;
    }
    const float gx = gfx - 0.5f, gy = gfy - 0.5f;
    if (!(gx > -1.0f && gx < (float)T.prev.W && gy > -1.0f && gy < (float)T.prev.H)) ok = false;      // no tap inside (or NaN)
    if (ok) {
      const float flx = floorf(gx), fly = floorf(gy);
      const int ix = (int)flx, iy = (int)fly;
      const float ax = gx - flx, ay = gy - fly;
      const size_t NP = (size_t)T.prev.W * (size_t)T.prev.H;
      for (int t = 0; t < 4; ++t) {
        const int ddx = t & 1, ddy = t >> 1;
        const int qx = ix + ddx, qy = iy + ddy;
        const float w = (ddx ? ax : 1.0f - ax) * (ddy ? ay : 1.0f - ay);
        if (!(w > 0.0f)) continue;
        if (qx < 0 || qx >= T.prev.W || qy < 0 || qy >= T.prev.H) continue;
        const size_t q = (size_t)qy * (size_t)T.prev.W + (size_t)qx;
        const Rec4 a = hist[q], b = hist[NP + q], c = hist[2 * NP + q];
        if (!(finite_f(a.x) && finite_f(a.y) && finite_f(a.z) && finite_f(a.w) && a.w > 0.0f)) continue;
        if (!(finite_f(b.x) && finite_f(b.y) && finite_f(b.z) && finite_f(c.x) && finite_f(c.y) && finite_f(c.z))) continue;
        if (T.has_depth && !(fabsf(b.z - e) <= T.depth_tol * e)) continue;
        if (T.has_normal && !(tp::dot3(nx, ny, nz, c.x, c.y, c.z) >= T.normal_min)) continue;
        if (T.has_id && __builtin_bit_cast(int32_t, b.w) != pid) continue;
        hr += w * a.x; hg += w * a.y; hb += w * a.z; hn += w * a.w; hm1 += w * b.x; hm2 += w * b.y;
        wsum += w;
      }
    }
  }

  // ---- C. combine, D. the outputs
  Out o;
  o.fallback = 0;
  o.h1.z = z; o.h1.w = __builtin_bit_cast(float, pid);
  o.h2.x = nx; o.h2.y = ny; o.h2.z = nz; o.h2.w = 0.0f;
  if (wsum > 0.0f) {
    hr = hr / wsum; hg = hg / wsum; hb = hb / wsum; hn = hn / wsum; hm1 = hm1 / wsum; hm2 = hm2 / wsum;
    if (K > 0.0f) {
      const float n_eff = kappa * T.n_cur;
      const float cr = kr / K, cg = kg / K, cb = kb / K, m1 = km1 / K, m2 = km2 / K;
      const float cap = T.max_history - n_eff;
      const float f = (hn > cap) ? cap / hn : 1.0f;
      const float n_new = n_eff + f * hn;
      const float a = n_eff / n_new, b = 1.0f - a;
      o.h0.x = a * cr + b * hr; o.h0.y = a * cg + b * hg; o.h0.z = a * cb + b * hb; o.h0.w = n_new;
      o.h1.x = a * m1 + b * hm1; o.h1.y = a * m2 + b * hm2;
    } else {                                                       // nothing of this frame lands here: the history is carried, no 0 * x is formed
      const float f = (hn > T.max_history) ? T.max_history / hn : 1.0f;
      o.h0.x = hr; o.h0.y = hg; o.h0.z = hb; o.h0.w = f * hn;
      o.h1.x = hm1; o.h1.y = hm2;
    }
  } else if (Hs > 0.0f) {
    o.h0.x = er / Hs; o.h0.y = eg / Hs; o.h0.z = eb / Hs; o.h0.w = T.n_cur * amax(kappa, P.min_confidence);
    o.h1.x = em1 / Hs; o.h1.y = em2 / Hs;
  } else if (Ua > 0.0f) {
    o.h0.x = ur / Ua; o.h0.y = ug / Ua; o.h0.z = ub / Ua; o.h0.w = T.n_cur * P.min_confidence;
    o.h1.x = um1 / Ua; o.h1.y = um2 / Ua;
    o.fallback = 1;
  } else {
    o.h0.x = o.h0.y = o.h0.z = o.h0.w = 0.0f;
    o.h1.x = o.h1.y = 0.0f;
    o.fallback = 2;
  }
  if (o.h0.w < 2.0f) {
    o.variance = __builtin_bit_cast(float, 0x7f800000u);
  } else {
    const double n = (double)o.h0.w, dm1 = (double)o.h1.x;
    const double D = (double)o.h1.y - dm1 * dm1;
    o.variance = (float)((((D < 0.0) ? 0.0 : D) * (n / (n - 1.0))) / n);
  }
  return o;
}

// ---- the ABI's parameters and the pointers -> Params: every refusal that needs no device.  Returns nullptr, or why the call is refused.
// The library (art_device_entries.cpp) and tests/temporal_upsample_host both derive their Params here.
inline const char* params_from_abi(const ArtTemporalUpsampleParams* p, const void* lo_color3f, const void* lo_moments2f, const ArtTemporalUpsampleGuides* lo,
                                   const ArtTemporalUpsampleGuides* hi, const void* hist_in, const void* hist_out, Params& P) {
  if (!p) return "null ArtTemporalUpsampleParams";
  if (!lo_color3f || !lo_moments2f || !hist_out) return "null lo_color3f, lo_moments2f or hist_out";
  if (!lo || !hi) return "null ArtTemporalUpsampleGuides (lo or hi)";
  if ((lo->normal3f != nullptr) != (hi->normal3f != nullptr)) return "normal3f is given on one side only";
  if ((lo->depth != nullptr) != (hi->depth != nullptr)) return "depth is given on one side only";
  if ((lo->id != nullptr) != (hi->id != nullptr)) return "id is given on one side only";
  if (lo->motion3f) return "lo motion3f must be NULL (the motion plane is the hi frame's)";
  if (const char* why = tp::params_from_abi(&p->t, lo_color3f, lo_moments2f, hi->normal3f, hi->depth, hi->id, hist_in, hist_out, P.T, hi->motion3f)) return why;
  const int32_t W = p->t.cur.width, H = p->t.cur.height;
  if (p->lo_width < 1 || p->lo_width > W || p->lo_height < 1 || p->lo_height > H) return "lo_width must be 1 .. width and lo_height 1 .. height";
  for (int k = 0; k < 2; ++k)
    if (!(p->jitter[k] > -0.5f && p->jitter[k] < 0.5f)) return "each jitter must be inside (-0.5, 0.5)";
  const float rx = (float)W / (float)p->lo_width, ry = (float)H / (float)p->lo_height;
  if (!(p->radius > 0.0f && p->radius <= (rx < ry ? rx : ry))) return "radius must be inside (0, min(width / lo_width, height / lo_height)]";
  if (!(p->min_confidence > 0.0f && p->min_confidence <= 1.0f)) return "min_confidence must be inside (0, 1]";
  P.LW = p->lo_width; P.LH = p->lo_height;
  P.jx = p->jitter[0]; P.jy = p->jitter[1]; P.radius = p->radius; P.min_confidence = p->min_confidence;
  return nullptr;
}

// An output over an input plane, or over another output: lanes store while others still read.  (After the planes' own check; hist_in
// against hist_out is tp::params_from_abi's.)
inline const char* overlap_refusal(const Params& P, const void* lo_color3f, const void* lo_moments2f, const ArtTemporalUpsampleGuides* lo,
                                   const ArtTemporalUpsampleGuides* hi, const void* hist_in, const void* hist_out, const void* out3f, const void* variance_out,
                                   const void* length_out, const void* fallback1b) {
  const size_t N = (size_t)P.T.cur.W * (size_t)P.T.cur.H, NL = (size_t)P.LW * (size_t)P.LH, NP = (size_t)P.T.prev.W * (size_t)P.T.prev.H;
  struct Plane { const void* p; size_t bytes; const char* what; };
  const Plane in[] = {{lo_color3f, 12 * NL, "lo_color3f"}, {lo_moments2f, 8 * NL, "lo_moments2f"}, {lo->normal3f, 12 * NL, "lo normal3f"}, {lo->depth, 4 * NL, "lo depth"},
                      {lo->id, 4 * NL, "lo id"}, {hi->normal3f, 12 * N, "hi normal3f"}, {hi->depth, 4 * N, "hi depth"}, {hi->id, 4 * N, "hi id"},
                      {hi->motion3f, 12 * N, "hi motion3f"}, {hist_in, 48 * NP, "hist_in"}};
  const Plane out[] = {{hist_out, 48 * N, "hist_out"}, {out3f, 12 * N, "out3f"}, {variance_out, 4 * N, "variance_out"}, {length_out, 4 * N, "length_out"}, {fallback1b, N, "fallback1b"}};
  auto overlap = [](const Plane& a, const Plane& b) {
    const char* x = (const char*)a.p; const char* y = (const char*)b.p;
    return a.p && b.p && x < y + b.bytes && y < x + a.bytes;
  };
  for (const Plane& o : out)
    for (const Plane& i : in)
      if (overlap(o, i)) return "an output overlaps an input plane";
  for (int a = 0; a < 5; ++a)
    for (int b = a + 1; b < 5; ++b)
      if (overlap(out[a], out[b])) return "two outputs overlap";
  return nullptr;
}

}  // namespace tu

// ---- launch interface (art_temporal_upsample.hip); hipcc only: the g++ build of the tests takes the text above and nothing else
#if defined(__HIPCC__)
// the caller's planes (nullptr: not given), the two histories and the library's scratch records, LW * LH of each
struct TemporalUpsampleArgs {
  tu::Params P;
  const float* lo_color; const float* lo_moments; const float* lo_normal; const float* lo_depth; const int32_t* lo_id;
  const float* normal; const float* depth; const int32_t* id; const float* motion;
  const tu::Rec4* hist_in; tu::Rec4* hist_out;
  float* out; float* variance_out; float* length_out; uint8_t* fallback;
  tu::Rec4* lo_a; tu::Rec4* lo_b; tu::Rec4* lo_c;
};
void launch_temporal_upsample(hipStream_t st, const TemporalUpsampleArgs& A);      // the pack kernel over the lo frame, then the kernel over the hi frame
#endif

}  // namespace art
