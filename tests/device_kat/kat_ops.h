// kat_ops.h -- TEST-ONLY: the per-element bodies of the known-answer ops, one item in, one item out, all binary32 words.
// Included by tests/device_kat/device_kat.hip (hipcc, gfx950: one item per lane) and by tests/host_sim/host_sim.cpp (g++: one item
// per loop turn).  Both call run_item() below, so the only difference between the two sides is the compiler -- which is what
// tests/test_gpu_device_kat.py measures.  Every op calls the PRODUCT's ART_HD functions (csrc/art_math.h, art_isect.h, art_shade.h)
// and does no arithmetic of its own.  tests/devkat.py holds the same table (op number, words in, words out, parameter bytes).
#pragma once
#include <string.h>
#include "../../ada-ray-tracer_amd/csrc/art_shade.h"

namespace kat {

using namespace art;

enum Op : int {
  // math
  OP_SINCOS = 0,        // x -> asincos_m1: s, c
  OP_TAN,               // x -> atan_m1(x), safe_tan(x)
  OP_APOW,              // x, y -> apow
  OP_SQRT,              // x -> sqrtf
  OP_RCP,               // x -> 1.0f / x
  OP_DIV,               // x, y -> x / y
  OP_NORMALIZE,         // a -> normalize(a)
  OP_REFLECT,           // d, n -> reflect(d, n)
  OP_PERPENDICULAR,     // a -> perpendicular(a)
  OP_LOG_POS,           // x (positive, finite) -> m1::log_pos((double)x): low word, high word
  OP_EXP_SMALL,         // t (|t| <= 200) -> m1::exp_small((double)t): low word, high word
  // sampling
  OP_SAMPLE_COSINE,     // r1, r2, direction, normal, power -> direction
  OP_SAMPLE_COSINE_FIXED,
  OP_FRESNEL,           // cos1, eta_ext, eta_int -> F
  OP_LIGHT_SAMPLE,      // u1, u2, p -> pos, dir, intensity, pdf          params: DevLight
  OP_LIGHT_EVAL_PDF,    // p, ray_dir, hit_dist -> pdf                    params: DevLight
  OP_SPHERE_LIGHT_PDF,  // p -> pdf                                       params: DevLight
  OP_PDF_AREA_TO_SOLID, // pdfA, dist, cos -> pdf
  OP_BSDF_SAMPLE,       // xi1, xi2, ray_dir, n -> color, dir, pdf, specular (0 / 1)     params: DevMaterial
  OP_BSDF_EVAL,         // l, v, n -> bxdf, pdf                           params: DevMaterial
  // hits
  OP_TRI_RAW,           // o, d, A, B, C -> t, u, v, accepted (0 / 1)
  OP_SPHERE,            // o, d, centre, radius -> t, key of the candidate (search bound kInfinity, index 0)
  OP_CORNELL,           // o, d -> slab_reference: hit (0 / 1), tmin, tmax; isect_cornell: t, key     params: cb_min[3], cb_max[3]
  OP_QUAD,              // o, d -> t, key                                 params: DevLight
  OP_SLAB,              // o, d, lo, hi, tbest -> slab_setup: inv, noi; slab_interval: tmn, tmx
  OP_CAND_WINS,         // t, key, best.t, best.key -> 0 / 1
  OP_SINCOS_F64,        // x -> m1::sincos((double)x) before its rounding to binary32: s low, high word, c low, high word
  // the two ends of a picture: the camera ray and the LDR frame
  OP_CAMERA_DIR,        // pixel, sample (as words) -> camera_dir                        params: CameraParams
  OP_RESOLVE,           // accum r, g, b, norm_c -> resolve_pixel (the packed word)
  OP_ROUND_U32,         // v (below 2^32: a larger value has no uint32_t) -> ada_round_u32 (as a word)
  OP_COLOUR_LUM,        // r, g, b -> colour_lum
  OP_COUNT
};

struct OpShape { int in_words, out_words, param_bytes; };
struct CameraParams { int32_t width, height, aa_on; float cam_z; float cam_matrix[16]; };     // what camera_dir reads of DevFrame / DevScene

ART_HD OpShape op_shape(int op) {
  switch (op) {
    case OP_SINCOS:              return {1, 2, 0};
    case OP_TAN:                 return {1, 2, 0};
    case OP_APOW:                return {2, 1, 0};
    case OP_SQRT:                return {1, 1, 0};
    case OP_RCP:                 return {1, 1, 0};
    case OP_DIV:                 return {2, 1, 0};
    case OP_NORMALIZE:           return {3, 3, 0};
    case OP_REFLECT:             return {6, 3, 0};
    case OP_PERPENDICULAR:       return {3, 3, 0};
    case OP_LOG_POS:             return {1, 2, 0};
    case OP_EXP_SMALL:           return {1, 2, 0};
    case OP_SAMPLE_COSINE:       return {9, 3, 0};
    case OP_SAMPLE_COSINE_FIXED: return {9, 3, 0};
    case OP_FRESNEL:             return {3, 1, 0};
    case OP_LIGHT_SAMPLE:        return {5, 10, (int)sizeof(DevLight)};
    case OP_LIGHT_EVAL_PDF:      return {7, 1, (int)sizeof(DevLight)};
    case OP_SPHERE_LIGHT_PDF:    return {3, 1, (int)sizeof(DevLight)};
    case OP_PDF_AREA_TO_SOLID:   return {3, 1, 0};
    case OP_BSDF_SAMPLE:         return {8, 8, (int)sizeof(DevMaterial)};
    case OP_BSDF_EVAL:           return {9, 4, (int)sizeof(DevMaterial)};
    case OP_TRI_RAW:             return {15, 4, 0};
    case OP_SPHERE:              return {10, 2, 0};
    case OP_CORNELL:             return {6, 5, 24};
    case OP_QUAD:                return {6, 2, (int)sizeof(DevLight)};
    case OP_SLAB:                return {13, 8, 0};
    case OP_CAND_WINS:           return {4, 1, 0};
    case OP_SINCOS_F64:          return {1, 4, 0};
    case OP_CAMERA_DIR:          return {2, 3, (int)sizeof(CameraParams)};
    case OP_RESOLVE:             return {4, 1, 0};
    case OP_ROUND_U32:           return {1, 1, 0};
    case OP_COLOUR_LUM:          return {3, 1, 0};
    default:                     return {0, 0, 0};
  }
}

ART_HD void put3(float* o, f3 v) { o[0] = v.x; o[1] = v.y; o[2] = v.z; }
ART_HD void put_f64(float* o, double v) {
  const uint64_t b = __builtin_bit_cast(uint64_t, v);
  o[0] = __builtin_bit_cast(float, (uint32_t)b); o[1] = __builtin_bit_cast(float, (uint32_t)(b >> 32));
}
ART_HD float flag(bool b) { return b ? 1.0f : 0.0f; }
ART_HD uint32_t word(float x) { return __builtin_bit_cast(uint32_t, x); }
ART_HD float as_float(uint32_t x) { return __builtin_bit_cast(float, x); }

// one item of op `op`: in[op_shape(op).in_words] -> out[op_shape(op).out_words]; params: op_shape(op).param_bytes bytes, 4-byte aligned
ART_HD void run_item(int op, const float* in, float* out, const void* params) {
  switch (op) {
    case OP_SINCOS: { float s, c; asincos_m1(in[0], s, c); out[0] = s; out[1] = c; return; }
    case OP_TAN: { out[0] = atan_m1(in[0]); out[1] = safe_tan(in[0]); return; }
    case OP_APOW: { out[0] = apow(in[0], in[1]); return; }
    case OP_SQRT: { out[0] = sqrtf(in[0]); return; }
    case OP_RCP: { out[0] = 1.0f / in[0]; return; }
    case OP_DIV: { out[0] = in[0] / in[1]; return; }
    case OP_NORMALIZE: { put3(out, normalize(ld3(in))); return; }
    case OP_REFLECT: { put3(out, reflect(ld3(in), ld3(in + 3))); return; }
    case OP_PERPENDICULAR: { put3(out, perpendicular(ld3(in))); return; }
    case OP_LOG_POS: { put_f64(out, m1::log_pos((double)in[0])); return; }
    case OP_EXP_SMALL: { put_f64(out, m1::exp_small((double)in[0])); return; }
    case OP_SAMPLE_COSINE: { put3(out, sample_cosine(in[0], in[1], ld3(in + 2), ld3(in + 5), in[8])); return; }
    case OP_SAMPLE_COSINE_FIXED: { put3(out, sample_cosine_fixed(in[0], in[1], ld3(in + 2), ld3(in + 5), in[8])); return; }
    case OP_FRESNEL: { out[0] = fresnel_unpolarised(in[0], in[1], in[2]); return; }
    case OP_LIGHT_SAMPLE: {
      const LightSample r = light_sample((const DevLight*)params, in[0], in[1], ld3(in + 2));
      put3(out, r.pos); put3(out + 3, r.dir); put3(out + 6, r.intensity); out[9] = r.pdf;
      return;
    }
    case OP_LIGHT_EVAL_PDF: { out[0] = light_eval_pdf((const DevLight*)params, ld3(in), ld3(in + 3), in[6]); return; }
    case OP_SPHERE_LIGHT_PDF: { out[0] = sphere_light_pdf((const DevLight*)params, ld3(in)); return; }
    case OP_PDF_AREA_TO_SOLID: { out[0] = pdf_area_to_solid(in[0], in[1], in[2]); return; }
    case OP_BSDF_SAMPLE: {
      const BsdfSample r = bsdf_sample(*(const DevMaterial*)params, in[0], in[1], ld3(in + 2), ld3(in + 5));
      put3(out, r.color); put3(out + 3, r.dir); out[6] = r.pdf; out[7] = flag(r.specular);
      return;
    }
    case OP_BSDF_EVAL: {
      f3 b; float pdf;
      bsdf_eval(*(const DevMaterial*)params, ld3(in), ld3(in + 3), ld3(in + 6), b, pdf);
      put3(out, b); out[3] = pdf;
      return;
    }
    case OP_TRI_RAW: {
      float t, u, v;
      const bool ok = tri_raw(ld3(in), ld3(in + 3), ld3(in + 6), ld3(in + 9), ld3(in + 12), t, u, v);
      out[0] = t; out[1] = u; out[2] = v; out[3] = flag(ok);
      return;
    }
    case OP_SPHERE: {
      Cand best = cand_init(kInfinity);
      DevSphere s; s.x = in[6]; s.y = in[7]; s.z = in[8]; s.r = in[9];
      isect_sphere(ld3(in), ld3(in + 3), s, 0u, best);
      out[0] = best.t; out[1] = as_float(best.key);
      return;
    }
    case OP_CORNELL: {
      DevScene s; memset(&s, 0, sizeof s);
      const float* b = (const float*)params;
      for (int k = 0; k < 3; ++k) { s.cb_min[k] = b[k]; s.cb_max[k] = b[3 + k]; }
      const f3 o = ld3(in), d = ld3(in + 3), rcp = ray_rcp(d);
      float tmin, tmax;
      out[0] = flag(slab_reference(o, rcp, s.cb_min, s.cb_max, tmin, tmax)); out[1] = tmin; out[2] = tmax;
      Cand best = cand_init(kInfinity);
      isect_cornell(o, d, rcp, s, best);
      out[3] = best.t; out[4] = as_float(best.key);
      return;
    }
    case OP_QUAD: {
      Cand best = cand_init(kInfinity);
      isect_quad(ld3(in), ld3(in + 3), (const DevLight*)params, 0u, best);
      out[0] = best.t; out[1] = as_float(best.key);
      return;
    }
    case OP_SLAB: {
      f3 inv, noi; float tmn, tmx;
      slab_setup(ld3(in), ld3(in + 3), inv, noi);
      slab_interval(ld3(in + 6), ld3(in + 9), inv, noi, in[12], tmn, tmx);
      put3(out, inv); put3(out + 3, noi); out[6] = tmn; out[7] = tmx;
      return;
    }
    case OP_CAND_WINS: {
      Cand b; b.t = in[2]; b.key = word(in[3]); b.u = 0.0f; b.v = 0.0f;
      out[0] = flag(cand_wins(in[0], word(in[1]), b));
      return;
    }
    case OP_SINCOS_F64: { double sd, cd; m1::sincos((double)in[0], sd, cd); put_f64(out, sd); put_f64(out + 2, cd); return; }
    case OP_CAMERA_DIR: {
      const CameraParams* c = (const CameraParams*)params;
      DevFrame fr; memset(&fr, 0, sizeof fr);
      DevScene s; memset(&s, 0, sizeof s);
      fr.width = c->width; fr.height = c->height; fr.aa_on = c->aa_on; fr.cam_z = c->cam_z;
      for (int k = 0; k < 16; ++k) s.cam_matrix[k] = c->cam_matrix[k];
      put3(out, camera_dir(fr, s, word(in[0]), word(in[1])));
      return;
    }
    case OP_RESOLVE: { out[0] = as_float(resolve_pixel(ld3(in), in[3])); return; }
    case OP_ROUND_U32: { out[0] = as_float(ada_round_u32(in[0])); return; }
    case OP_COLOUR_LUM: { out[0] = colour_lum(ld3(in)); return; }
    default: return;
  }
}

}  // namespace kat
