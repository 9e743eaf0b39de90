// art_temporal.h -- the per-pixel text of art_temporal_device (include/art_hip.h states the arithmetic; this is its one definition).
// ART_HD functions over plain pointers, no HIP types: art_temporal.hip compiles them for gfx950 and tests/temporal_host compiles the same
// text with g++ (the arrangement of art_denoise.h with tests/denoise_host), so the kernel and the host build cannot drift apart.
//
// The history (the caller's, one in and one out) is three planes of 16-byte records per pixel, row-major, plane k at records k * W * H ..:
//   plane 0  Rec4 {r, g, b, n}        the mean colour and the history length in colours
//   plane 1  Rec4 {m1, m2, z, id}     the mean luminance, the mean squared luminance, the frame's depth and id (the id's int32 as a word)
//   plane 2  Rec4 {nx, ny, nz, 0}     the frame's normal
// so a tap costs three 16-byte loads.
#pragma once
#include <string.h>
#include "art_hip.h"
#include "art_denoise.h"

namespace art {
namespace tp {

using dn::Rec4;
using dn::finite_f;

// one camera as the kernel needs it: the host derives cam_z as make_frame does and inverts the 3 x 3 in binary64 (camera_from_abi)
struct Cam {
  float pos[3];
  float m[9];                      // the 3 x 3 of cam_matrix, row-major (rows 0..2, columns 0..2)
  float minv[9];                   // its inverse, each element rounded once from binary64
  float cam_z;
  int32_t W, H;
};

struct Params {
  Cam cur, prev;
  int32_t has_hist, has_normal, has_depth, has_id;
  int32_t reproject;               // 0: every pixel maps to itself (no depth plane, or the two cameras are the same words)
  float n_cur, max_history;        // (float)n_colours, (float)max_history
  float scale, depth_tol, normal_min;
};

// T = safe_tan(kHalfPi / 2.0f), what make_frame divides by (art_render.cpp); the header states its value
ART_HD float cam_z_of(int32_t width) { return -(float)width / safe_tan(kHalfPi / 2.0f); }

// cam_matrix's 3 x 3 and its inverse by the adjugate, in binary64, each element rounded once to binary32.  false: the matrix is refused
// (an element or the position not finite, a translation column that is not zero, a determinant that is zero or not finite, an inverse
// element that is not finite in binary32).
inline bool camera_from_abi(const float* cam_pos, const float* cam_matrix, int32_t width, int32_t height, Cam& c) {
  for (int k = 0; k < 3; ++k) { if (!finite_f(cam_pos[k])) return false; c.pos[k] = cam_pos[k]; }
  for (int k = 0; k < 16; ++k) if (!finite_f(cam_matrix[k])) return false;
  if (cam_matrix[3] != 0.0f || cam_matrix[7] != 0.0f || cam_matrix[11] != 0.0f) return false;
  double a[3][3];
  for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) { c.m[3 * r + k] = cam_matrix[4 * r + k]; a[r][k] = (double)cam_matrix[4 * r + k]; }
  const double c00 = a[1][1] * a[2][2] - a[1][2] * a[2][1], c01 = a[1][0] * a[2][2] - a[1][2] * a[2][0], c02 = a[1][0] * a[2][1] - a[1][1] * a[2][0];
  const double det = (a[0][0] * c00 - a[0][1] * c01) + a[0][2] * c02;
  if (!(det != 0.0) || !(det - det == 0.0)) return false;
  const double inv[9] = {
      c00 / det, (a[0][2] * a[2][1] - a[0][1] * a[2][2]) / det, (a[0][1] * a[1][2] - a[0][2] * a[1][1]) / det,
      (a[1][2] * a[2][0] - a[1][0] * a[2][2]) / det, (a[0][0] * a[2][2] - a[0][2] * a[2][0]) / det, (a[0][2] * a[1][0] - a[0][0] * a[1][2]) / det,
      c02 / det, (a[0][1] * a[2][0] - a[0][0] * a[2][1]) / det, (a[0][0] * a[1][1] - a[0][1] * a[1][0]) / det};
  for (int k = 0; k < 9; ++k) { c.minv[k] = (float)inv[k]; if (!finite_f(c.minv[k])) return false; }
  c.cam_z = cam_z_of(width); c.W = width; c.H = height;
  return true;
}

// ArtTemporalParams and which pointers are given -> the kernel's Params: every refusal that needs no device, the two cameras, and the rule
// of step 3 (no reprojection without depth, without history, or between cameras that are the same words).  Returns nullptr, or why the
// call is refused.  The library (art_device_entries.cpp) and tests/temporal_host both derive their Params here.
// motion3f: art_temporal_motion_device's plane (nullptr: art_temporal_device's rules, word for word).
inline const char* params_from_abi(const ArtTemporalParams* p, const void* color3f, const void* moments2f, const void* normal3f, const void* depth, const void* id,
                                   const void* hist_in, const void* hist_out, Params& P, const void* motion3f = nullptr) {
  if (!p) return "null ArtTemporalParams";
  if (!color3f || !moments2f || !hist_out) return "null color3f, moments2f or hist_out";
  const ArtTemporalCamera& cc = p->cur; const ArtTemporalCamera& pc = p->prev;
  if (cc.width < 1 || cc.height < 1 || (int64_t)cc.width * cc.height > (1ll << 28)) return "cur: width and height must be at least 1 and width * height at most 2^28";
  if (hist_in && (pc.width < 1 || pc.height < 1 || (int64_t)pc.width * pc.height > (1ll << 28))) return "prev: width and height must be at least 1 and width * height at most 2^28";
  if (p->n_colours < 1) return "n_colours must be at least 1";
  if (p->max_history < p->n_colours || p->max_history > (1 << 24)) return "max_history must be n_colours .. 2^24";
  if (!finite_f(p->scale)) return "scale is not finite";
  if (p->depth_tol != p->depth_tol || p->normal_min != p->normal_min) return "depth_tol or normal_min is NaN";
  memset(&P, 0, sizeof P);
  if (!camera_from_abi(cc.cam_pos, cc.cam_matrix, cc.width, cc.height, P.cur))
    return "cur: the camera is refused (a component that is not finite, a translation column m[3], m[7], m[11] that is not zero, or a singular 3 x 3)";
  if (hist_in) {
    if (!camera_from_abi(pc.cam_pos, pc.cam_matrix, pc.width, pc.height, P.prev))
      return "prev: the camera is refused (a component that is not finite, a translation column m[3], m[7], m[11] that is not zero, or a singular 3 x 3)";
  } else {
    P.prev = P.cur;
  }
  if (hist_in) {
    const size_t N = (size_t)cc.width * (size_t)cc.height, NP = (size_t)pc.width * (size_t)pc.height;
    const char* a = (const char*)hist_in; const char* b = (const char*)hist_out;
    if (a < b + 48 * N && b < a + 48 * NP) return "hist_in and hist_out overlap";
  }
  P.has_hist = hist_in ? 1 : 0; P.has_normal = normal3f ? 1 : 0; P.has_depth = depth ? 1 : 0; P.has_id = id ? 1 : 0;
  const bool same = memcmp(cc.cam_pos, pc.cam_pos, 12) == 0 && memcmp(cc.cam_matrix, pc.cam_matrix, 64) == 0 && cc.width == pc.width && cc.height == pc.height;
  P.reproject = (depth && hist_in && !same) ? 1 : 0;
  if (motion3f) P.reproject = (depth && hist_in) ? 1 : 0;      // a surface may have moved under cameras at rest
  P.n_cur = (float)p->n_colours; P.max_history = (float)p->max_history;
  P.scale = p->scale; P.depth_tol = p->depth_tol; P.normal_min = p->normal_min;
  return nullptr;
}

ART_HD float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

struct Out { Rec4 h0, h1, h2; float variance; };

// pixel (x, y) of the current frame: its three history records and the variance of its mean luminance (h0 holds out3f and length_out).
// MOTION (art_temporal_motion_device with a motion plane; P comes from params_from_abi with that plane named): the world point of step 3
// is taken back by the pixel's delta.  Without it motion is not read: the text is art_temporal_device's.
template <bool MOTION = false>
ART_HD Out temporal_pixel(const Params& P, const float* color, const float* moments, const float* normal, const float* depth, const int32_t* id,
                          const Rec4* hist, int x, int y, const float* motion = nullptr) {
  const size_t p = (size_t)y * (size_t)P.cur.W + (size_t)x;
  const float cr = P.scale * color[3 * p], cg = P.scale * color[3 * p + 1], cb = P.scale * color[3 * p + 2];
  const float m1 = moments[2 * p] / P.n_cur, m2 = moments[2 * p + 1] / P.n_cur;
  const float z = P.has_depth ? depth[p] : 0.0f;
  const int32_t pid = P.has_id ? id[p] : 0;
  float nx = 0.0f, ny = 0.0f, nz = 0.0f;
  if (P.has_normal) { nx = normal[3 * p]; ny = normal[3 * p + 1]; nz = normal[3 * p + 2]; }
  bool own = !P.has_hist;
  if (P.has_depth && !(z > 0.0f && finite_f(z))) own = true;
  if (P.has_normal && !(finite_f(nx) && finite_f(ny) && finite_f(nz))) own = true;

  float hr = 0.0f, hg = 0.0f, hb = 0.0f, hn = 0.0f, hm1 = 0.0f, hm2 = 0.0f, wsum = 0.0f;
  if (!own) {
    float fx = (float)x + 0.5f, fy = (float)y + 0.5f, e = z;
    bool ok = true;
    if (P.reproject) {
      const float rx = ((float)x + 0.5f) - ((float)P.cur.W / 2.0f), ry = ((float)y + 0.5f) - ((float)P.cur.H / 2.0f), rz = P.cur.cam_z;
      const float li = 1.0f / sqrtf(dot3(rx, ry, rz, rx, ry, rz));
      const float ux = li * rx, uy = li * ry, uz = li * rz;
      const float* M = P.cur.m;
      const float tx = (M[0] * ux + M[1] * uy) + M[2] * uz, ty = (M[3] * ux + M[4] * uy) + M[5] * uz, tz = (M[6] * ux + M[7] * uy) + M[8] * uz;
      const float lj = 1.0f / sqrtf(dot3(tx, ty, tz, tx, ty, tz));
      const float dx = lj * tx, dy = lj * ty, dz = lj * tz;
      float vx, vy, vz;
      if constexpr (MOTION) {
        const float mx = motion[3 * p], my = motion[3 * p + 1], mz = motion[3 * p + 2];
        if (!(finite_f(mx) && finite_f(my) && finite_f(mz))) ok = false;
        vx = ((P.cur.pos[0] + z * dx) + mx) - P.prev.pos[0]; vy = ((P.cur.pos[1] + z * dy) + my) - P.prev.pos[1]; vz = ((P.cur.pos[2] + z * dz) + mz) - P.prev.pos[2];
      } else {
        vx = (P.cur.pos[0] + z * dx) - P.prev.pos[0]; vy = (P.cur.pos[1] + z * dy) - P.prev.pos[1]; vz = (P.cur.pos[2] + z * dz) - P.prev.pos[2];
      }
      e = sqrtf(dot3(vx, vy, vz, vx, vy, vz));
      const float* I = P.prev.minv;
      const float qx = (I[0] * vx + I[1] * vy) + I[2] * vz, qy = (I[3] * vx + I[4] * vy) + I[5] * vz, qz = (I[6] * vx + I[7] * vy) + I[8] * vz;
      if (!(qz * P.prev.cam_z > 0.0f)) ok = false;               // behind the previous camera, or NaN
      const float k = P.prev.cam_z / qz;
      fx = qx * k + (float)P.prev.W / 2.0f; fy = qy * k + (float)P.prev.H / 2.0f;
    }
    const float gx = fx - 0.5f, gy = fy - 0.5f;
    if (!(gx > -1.0f && gx < (float)P.prev.W && gy > -1.0f && gy < (float)P.prev.H)) ok = false;      // no tap inside (or NaN)
    if (ok) {
      const float flx = floorf(gx), fly = floorf(gy);
      const int ix = (int)flx, iy = (int)fly;
      const float ax = gx - flx, ay = gy - fly;
      const size_t NP = (size_t)P.prev.W * (size_t)P.prev.H;
      for (int t = 0; t < 4; ++t) {
        const int ddx = t & 1, ddy = t >> 1;
        const int qx = ix + ddx, qy = iy + ddy;
        const float w = (ddx ? ax : 1.0f - ax) * (ddy ? ay : 1.0f - ay);
        if (!(w > 0.0f)) continue;
        if (qx < 0 || qx >= P.prev.W || qy < 0 || qy >= P.prev.H) continue;
        const size_t q = (size_t)qy * (size_t)P.prev.W + (size_t)qx;
        const Rec4 a = hist[q], b = hist[NP + q], c = hist[2 * NP + q];
        if (!(finite_f(a.x) && finite_f(a.y) && finite_f(a.z) && finite_f(a.w) && a.w > 0.0f)) continue;
        if (!(finite_f(b.x) && finite_f(b.y) && finite_f(b.z) && finite_f(c.x) && finite_f(c.y) && finite_f(c.z))) continue;
        if (P.has_depth && !(fabsf(b.z - e) <= P.depth_tol * e)) continue;
        if (P.has_normal && !(dot3(nx, ny, nz, c.x, c.y, c.z) >= P.normal_min)) continue;
        if (P.has_id && __builtin_bit_cast(int32_t, b.w) != pid) continue;
        hr += w * a.x; hg += w * a.y; hb += w * a.z; hn += w * a.w; hm1 += w * b.x; hm2 += w * b.y;
        wsum += w;
      }
    }
  }
  Out o;
  o.h0.x = cr; o.h0.y = cg; o.h0.z = cb; o.h0.w = P.n_cur;
  o.h1.x = m1; o.h1.y = m2; o.h1.z = z; o.h1.w = __builtin_bit_cast(float, pid);
  o.h2.x = nx; o.h2.y = ny; o.h2.z = nz; o.h2.w = 0.0f;
  if (wsum > 0.0f) {
    hr = hr / wsum; hg = hg / wsum; hb = hb / wsum; hn = hn / wsum; hm1 = hm1 / wsum; hm2 = hm2 / wsum;
    const float cap = P.max_history - P.n_cur;
    const float f = (hn > cap) ? cap / hn : 1.0f;
    const float n_new = P.n_cur + f * hn;
    const float a = P.n_cur / n_new, b = 1.0f - a;
    o.h0.x = a * cr + b * hr; o.h0.y = a * cg + b * hg; o.h0.z = a * cb + b * hb; o.h0.w = n_new;
    o.h1.x = a * m1 + b * hm1; o.h1.y = a * m2 + b * hm2;
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

}  // namespace tp

// ---- launch interface (art_temporal.hip); hipcc only: the g++ builds of the tests take the per-pixel text above and nothing else
#if defined(__HIPCC__)
// art_temporal_device (art_temporal.hip, art_device_entries.cpp temporal_device): the caller's current planes (normal / depth / id nullptr: not given),
// the two histories (hist_in nullptr: the first frame) and the optional outputs; n = W * H of the current frame
struct TemporalArgs {
  tp::Params P;
  int32_t n;
  int32_t has_motion;              // art_temporal_motion_device with a motion plane: the MOTION instantiation runs (the word lies in what was padding)
  const float* color; const float* moments; const float* normal; const float* depth; const int32_t* id;
  const tp::Rec4* hist_in; tp::Rec4* hist_out;
  float* out; float* variance_out; float* length_out;
  const float* motion;             // art_temporal_motion_device: 3 floats per pixel of the current frame; else nullptr
};
void launch_temporal(hipStream_t st, const TemporalArgs& A);      // A.has_motion selects the motion variant of the kernel
#endif

}  // namespace art
