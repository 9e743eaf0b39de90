// TEST-ONLY: art_denoise_device on host arrays, through the product's own per-pixel text (csrc/art_denoise.h) compiled by g++.  The
// argument rules are the ABI's (include/art_hip.h); pointers are host memory; out3f may be color3f.  Returns 0, or 1 for a refused argument.
#include "art_hip.h"
#include "filter_host.h"

using namespace art;

extern "C" int dh_denoise(const ArtDenoiseParams* p, const float* color3f, const float* albedo3f, const float* normal3f, const float* depth, float* out3f) {
  dn::Params P;
  if (dn::params_from_abi(p, color3f, albedo3f, normal3f, depth, out3f, P)) return 1;      // (the library's own derivation and refusals)
  filter_host<dn::Mode::Plain>(P, p->iterations, 0, color3f, nullptr, albedo3f, normal3f, depth, out3f, nullptr);
  return 0;
}
