// TEST-ONLY: the per-item functions of art_radiance_rays_device (csrc/art_radiance.h: raygen_ray_slot, accumulate_ray) compiled by g++ as a
// stand-alone program (tests/test_radiance_reference_host.py builds it plain and with AddressSanitizer + UBSan, runs both and holds their
// output to tests/radiance_ref.py).
//   radiance_host                 the program's own checks
//   radiance_host in.bin out.bin  in: int32 mode, n, samples, chunk, has_moments, then
//     mode 0 (accumulate): values [n][samples][3], radiance [n][3], moments [n][2]  ->  out: radiance [n][3], moments [n][2]; the samples go
//                          through accumulate_ray in batches of `chunk`, as a call cut into sample chunks does
//     mode 1 (raygen):     origins [n][3], dirs [n][3]  ->  out: int32 stride, then the bank's hot block, kHotFields * stride words, of the
//                          n * samples slots (slot = sample * n + ray) of a scene without analytic primitives and without a BVH
#include <cstdio>
#include <cstring>
#include <vector>

#include "art_radiance.h"

using namespace art;

static bool read_all(const char* path, std::vector<char>& buf) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  std::fseek(f, 0, SEEK_END); const long n = std::ftell(f); std::fseek(f, 0, SEEK_SET);
  buf.resize((size_t)n);
  const bool ok = n == 0 || std::fread(buf.data(), 1, (size_t)n, f) == (size_t)n;
  std::fclose(f);
  return ok;
}

static void accumulate(int n, int samples, int chunk, const float* values, float* radiance, float* moments) {
  for (int s0 = 0; s0 < samples; s0 += chunk) {
    const int sn = (samples - s0 < chunk) ? samples - s0 : chunk;
    std::vector<float> r((size_t)sn * n), g((size_t)sn * n), b((size_t)sn * n);
    for (int t = 0; t < sn; ++t)
      for (int i = 0; i < n; ++i) {
        const float* v = values + ((size_t)i * samples + (size_t)(s0 + t)) * 3;
        r[(size_t)t * n + i] = v[0]; g[(size_t)t * n + i] = v[1]; b[(size_t)t * n + i] = v[2];
      }
    DevPaths q; std::memset(&q, 0, sizeof q);
    q.P = sn * n; q.npix = n; q.rad_r = r.data(); q.rad_g = g.data(); q.rad_b = b.data();
    for (int i = 0; i < n; ++i) accumulate_ray(q, i, sn, radiance, moments);
  }
}

// the hot block raygen_ray_slot leaves; returns the stride
static int raygen(int n, int samples, const float* origins, const float* dirs, std::vector<uint32_t>& hot) {
  const int P = n * samples, stride = (P + 63) & ~63;
  hot.assign((size_t)kHotFields * stride, 0xDEADBEEFu);
  std::vector<Rec4> rec((size_t)P);
  DevScene s; std::memset(&s, 0, sizeof s);
  DevPaths q; std::memset(&q, 0, sizeof q);
  q.P = P; q.npix = n; q.hot = reinterpret_cast<float*>(hot.data()); q.stride = stride; q.rec = rec.data(); q.rec_mode = REC_EXT; q.has_bvh = 0;
  StageCtx cx; cx.hot_layout = true;
  for (int slot = 0; slot < P; ++slot) {
    const int i = slot % n;
    raygen_ray_slot(s, q, slot, mk3(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]), mk3(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]), cx);
  }
  return stride;
}

static int self_checks() {
  int bad = 0;
  {   // two paths of one ray: (1, 2, 3) then (0.5, 0.25, 0.125) into a plane that holds (10, 20, 30)
    const float values[6] = {1.0f, 2.0f, 3.0f, 0.5f, 0.25f, 0.125f};
    float rad[3] = {10.0f, 20.0f, 30.0f}, mom[2] = {0.0f, 0.0f};
    accumulate(1, 2, 2, values, rad, mom);
    bad += !(rad[0] == 11.5f && rad[1] == 22.25f && rad[2] == 33.125f);
    const float l0 = (0.2126f * 1.0f + 0.7152f * 2.0f) + 0.0722f * 3.0f, l1 = (0.2126f * 0.5f + 0.7152f * 0.25f) + 0.0722f * 0.125f;
    bad += !(mom[0] == l1 + (l0 + 0.0f) && mom[1] == l1 * l1 + (l0 * l0 + 0.0f));
    float rad1[3] = {10.0f, 20.0f, 30.0f};
    accumulate(1, 2, 1, values, rad1, nullptr);               // without moments, one sample per batch
    bad += !(rad1[0] == rad[0] && rad1[1] == rad[1] && rad1[2] == rad[2]);
  }
  {   // one ray, three samples: slots 0, 1, 2 hold the same ray; the padding of the block stays untouched
    const float o[3] = {1.0f, 2.0f, 3.0f}, d[3] = {0.0f, 0.0f, 2.0f};
    std::vector<uint32_t> hot;
    const int st = raygen(1, 3, o, d, hot);
    bad += !(st == 64);
    for (int slot = 0; slot < 3; ++slot) {
      float dz, pdf; std::memcpy(&dz, &hot[(size_t)HF_DZ * st + slot], 4); std::memcpy(&pdf, &hot[(size_t)HF_PDF * st + slot], 4);
      bad += !(dz == 2.0f && pdf == 1.0f && hot[(size_t)HF_FLAGS * st + slot] == (FLAG_ALIVE | FLAG_PREV_SPEC) && hot[(size_t)HF_SLOT * st + slot] == (uint32_t)slot);
      bad += !(hot[(size_t)HF_HIT * st + 4 * slot + 1] == KEY_MISS);
    }
    bad += !(hot[(size_t)HF_OX * st + 3] == 0xDEADBEEFu);
  }
  std::printf(bad ? "radiance_host: %d check(s) FAILED\n" : "radiance_host: ok\n", bad);
  return bad ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc == 1) return self_checks();
  if (argc != 3) { std::fprintf(stderr, "usage: radiance_host [in.bin out.bin]\n"); return 2; }
  std::vector<char> in;
  if (!read_all(argv[1], in) || in.size() < 20) { std::fprintf(stderr, "radiance_host: cannot read %s\n", argv[1]); return 2; }
  int32_t h[5]; std::memcpy(h, in.data(), 20);
  const int mode = h[0], n = h[1], samples = h[2], chunk = h[3], has_moments = h[4];
  if (n < 1 || samples < 1 || chunk < 1 || (mode != 0 && mode != 1)) { std::fprintf(stderr, "radiance_host: bad header\n"); return 2; }
  const size_t N = (size_t)n;
  const size_t want = 20 + 4 * (mode == 0 ? N * samples * 3 + N * 3 + N * 2 : N * 6);
  if (in.size() != want) { std::fprintf(stderr, "radiance_host: %zu bytes, expected %zu\n", in.size(), want); return 2; }
  std::vector<float> f((in.size() - 20) / 4);
  std::memcpy(f.data(), in.data() + 20, in.size() - 20);
  FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  if (mode == 0) {
    float* values = f.data(); float* rad = values + N * samples * 3; float* mom = rad + N * 3;
    accumulate(n, samples, chunk, values, rad, has_moments ? mom : nullptr);
    std::fwrite(rad, 4, N * 3, out); std::fwrite(mom, 4, N * 2, out);
  } else {
    std::vector<uint32_t> hot;
    const int32_t stride = raygen(n, samples, f.data(), f.data() + N * 3, hot);
    std::fwrite(&stride, 4, 1, out); std::fwrite(hot.data(), 4, hot.size(), out);
  }
  std::fclose(out);
  return 0;
}
