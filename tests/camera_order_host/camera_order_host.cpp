// TEST-ONLY: the visiting order of bounce 0 (csrc/art_camera_order.h, option camera_order) compiled by g++ as a stand-alone program for
// tests/test_camera_order_host.py.  The header needs no HIP.  The Makefile builds it with AddressSanitizer and UBSan.
//   camera_order_host PN SN   prints "units N", one line "u SLOT0 COUNT" per unit of the order, then "positions V unmasked M" from a walk
//                             over every visiting position through camera_order_slot, which must agree with the units
//   camera_order_host         the program's own checks over a few shapes; prints "camera_order_host: ok"
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../ada-ray-tracer_amd/csrc/art_camera_order.h"

using namespace art;

static int fail(const char* what, int pn, int sn, long long at) { std::printf("camera_order_host: %s (pn %d, sn %d, at %lld)\n", what, pn, sn, at); return 1; }

// every position through camera_order_slot: agrees with the unit it lies in, hits every slot exactly once
static int walk(int pn, int sn, long long* positions, long long* unmasked) {
  const int n_units = camera_order_units(pn, sn);
  std::vector<unsigned char> seen((size_t)pn * sn, 0);
  *positions = (long long)n_units * kOrderUnit; *unmasked = 0;
  for (long long v = 0; v < *positions; ++v) {
    const OrderUnit u = camera_order_unit(pn, sn, (int)(v / kOrderUnit));
    const int t = (int)(v % kOrderUnit), slot = camera_order_slot(pn, sn, v);
    if (slot != (t < u.count ? u.slot0 + t : -1)) return fail("position and unit disagree", pn, sn, v);
    if (slot < 0) continue;
    if (slot >= pn * sn) return fail("slot out of range", pn, sn, v);
    if (seen[(size_t)slot]++) return fail("slot visited twice", pn, sn, v);
    *unmasked += 1;
  }
  if (*unmasked != (long long)pn * sn) return fail("slots missed", pn, sn, *unmasked);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3) {
    const int pn = std::atoi(argv[1]), sn = std::atoi(argv[2]);
    if (pn < 1 || sn < 1 || (long long)pn * sn > (1ll << 27)) return fail("bad shape", pn, sn, 0);
    const int n_units = camera_order_units(pn, sn);
    std::printf("units %d\n", n_units);
    for (int u = 0; u < n_units; ++u) { const OrderUnit o = camera_order_unit(pn, sn, u); std::printf("u %d %d\n", o.slot0, o.count); }
    long long positions = 0, unmasked = 0;
    if (walk(pn, sn, &positions, &unmasked)) return 1;
    std::printf("positions %lld unmasked %lld\n", positions, unmasked);
    return 0;
  }
  const int shapes[][2] = {{1, 1}, {1, 4}, {256, 1}, {1023, 3}, {1024, 4}, {1025, 5}, {4096, 2}, {5000, 7}, {524288, 16}};
  for (const auto& s : shapes) {
    long long positions = 0, unmasked = 0;
    if (walk(s[0], s[1], &positions, &unmasked)) return 1;
    int last_block = 0;
    for (int u = 0; u < camera_order_units(s[0], s[1]); ++u) {
      const OrderUnit o = camera_order_unit(s[0], s[1], u);
      const int block = (o.slot0 % s[0]) / (kOrderUnit * kOrderBlockUnits);
      if (o.count < 1 || o.count > kOrderUnit || o.slot0 / s[0] != (o.slot0 + o.count - 1) / s[0]) return fail("a unit leaves its sample row", s[0], s[1], u);
      if (block < last_block) return fail("a block comes back", s[0], s[1], u);
      last_block = block;
    }
  }
  std::printf("camera_order_host: ok\n");
  return 0;
}
