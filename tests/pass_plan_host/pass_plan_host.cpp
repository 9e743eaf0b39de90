// TEST-ONLY: the render pass' host logic (csrc/art_pass_plan.h: plan_batch, ShadeTrial) compiled by g++, behind C functions for
// tests/test_pass_plan_host.py.  The header needs no HIP.
#include "../../ada-ray-tracer_amd/csrc/art_pass_plan.h"

using namespace art;

extern "C" {

void pp_plan_batch(int npix, int S, int per, int64_t cap, int* pc, int* sc) { const BatchPlan b = plan_batch(npix, S, per, cap); *pc = b.pc; *sc = b.sc; }

ShadeTrial* pp_trial_new() { return new ShadeTrial; }
void pp_trial_free(ShadeTrial* t) { delete t; }
void pp_trial_reset(ShadeTrial* t) { t->reset(); }
void pp_trial_next(ShadeTrial* t, int64_t paths, int pinned_option, int record_schedule, int* trial, int* shade_per) {
  const ShadeTrial::Batch b = t->next(paths, pinned_option, record_schedule != 0);
  *trial = b.trial; *shade_per = b.shade_per;
}
void pp_trial_add(ShadeTrial* t, int trial, unsigned gen, double ms) { t->add(trial, gen, ms); }
int pp_trial_decide(ShadeTrial* t) { return t->decide() ? 1 : 0; }
// phase, per, redo, gen | ms[0], ms[1]
void pp_trial_state(const ShadeTrial* t, int64_t* i4, double* ms2) { i4[0] = t->phase; i4[1] = t->per; i4[2] = t->redo; i4[3] = t->gen; ms2[0] = t->ms[0]; ms2[1] = t->ms[1]; }
int pp_trial_tag(const ShadeTrial* t, int kind, int trial) { return t->tag(kind, trial); }

int pp_tag_encode(int kind, int trial, unsigned gen) { return ShadeTrial::encode(kind, trial, gen); }
void pp_tag_decode(int tag, int* kind, int* trial, int* gen) { const ShadeTrial::Tag g = ShadeTrial::decode((uint8_t)tag); *kind = g.kind; *trial = g.trial; *gen = (int)g.gen; }

}  // extern "C"
