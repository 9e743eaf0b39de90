// art_camera_order.h -- the order in which bounce 0 of the compacted schedule (k_shade_compact<PER, true>) visits the path slots of a
// batch: option camera_order = 1.  Plain C++17 on the host (tests/camera_order_host compiles it with g++), __host__ __device__ under hipcc.
//
// Slots are sample-major (slot = sl * pn + pl: art_shade.h slot_split) and stay so.  What changes is only which slot a thread of bounce 0
// picks up, and with it the order in which the survivors reach the output bank and every later stage: all samples of a block of pixels
// before the next block, so that a contiguous piece of the trace kernel's queue holds the paths of one patch of the picture.
//   unit   256 consecutive slots of ONE sample row: pixels [256 q, min(256 q + 256, pn)) of sample s -- a round of k_shade_compact, which
//          must touch one 1-KB window of every slot-indexed array;
//   block  1024 consecutive pl = 4 units per sample row (one 32 x 32 tile of the pixel map when the context owns whole tiles); the last
//          block of a row has ceil((pn mod 1024) / 256) units, its last unit pn mod 256 slots;
//   order  block-major, then sample, then the block's units.
// The visiting space is 256 positions per unit, sn * ceil(pn / 256) units: larger than pn * sn when pn is no multiple of 256; the
// positions of a unit beyond its slots are padding and do no work.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define ART_ORDER_HD __host__ __device__ __forceinline__
#else
#define ART_ORDER_HD inline
#endif

namespace art {

constexpr int kOrderUnit = 256;             // slots per unit
constexpr int kOrderBlockUnits = 4;         // units of a sample row per pixel block

struct OrderUnit { int slot0, count; };     // the unit's first slot and its number of slots (1 .. 256)

// units of a batch of pn pixels x sn samples (pn * sn <= 2^27: at most 2^27 units)
ART_ORDER_HD int camera_order_units(int pn, int sn) { return sn * ((pn + kOrderUnit - 1) / kOrderUnit); }

// unit u of the visiting order, 0 <= u < camera_order_units(pn, sn).  Two integer divisions: on the device u is wave-uniform, so they are
// made once per round of a workgroup.
ART_ORDER_HD OrderUnit camera_order_unit(int pn, int sn, int u) {
  const int blk = kOrderUnit * kOrderBlockUnits;
  const int full = pn / blk;                                   // whole blocks: 4 units per sample row each
  int b = u / (kOrderBlockUnits * sn), r = u - b * (kOrderBlockUnits * sn);
  int upr = kOrderBlockUnits;                                  // units per sample row of this unit's block
  if (b >= full) {                                             // the partial last block: 1 .. 4 units per row
    b = full; r = u - full * (kOrderBlockUnits * sn);
    upr = (pn - full * blk + kOrderUnit - 1) / kOrderUnit;
  }
  const int s = r / upr, j = r - s * upr;
  const int pl0 = b * blk + j * kOrderUnit;
  OrderUnit o;
  o.slot0 = s * pn + pl0;
  o.count = (pn - pl0 < kOrderUnit) ? pn - pl0 : kOrderUnit;
  return o;
}

// visiting position v (0 <= v < 256 * camera_order_units) -> its slot, or -1 for padding
ART_ORDER_HD int camera_order_slot(int pn, int sn, int64_t v) {
  const OrderUnit o = camera_order_unit(pn, sn, (int)(v / kOrderUnit));
  const int t = (int)(v % kOrderUnit);
  return t < o.count ? o.slot0 + t : -1;
}

}  // namespace art
