// TEST-ONLY: the host logic of EventPairs (csrc/art_event_pairs.h) against counting stubs of the HIP event calls -- free-list reuse,
// rollback when the first record fails, cancel, a fold that keeps pairs in flight, the first-error rule of a waiting fold.  A stand-alone
// program for AddressSanitizer + UBSan on the CPU (tests/test_event_pairs.py builds and runs it); the stub events are heap cells, so a
// double destroy, a use after destroy or a leaked event is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <vector>

enum hipError_t { hipSuccess = 0, hipErrorInvalidHandle = 400, hipErrorNotReady = 600, hipErrorOutOfMemory = 2 };
struct StubEvent { bool recorded = false, done = false; float at = 0.0f; void* stream = nullptr; };
typedef StubEvent* hipEvent_t;
typedef void* hipStream_t;

static int g_created = 0, g_destroyed = 0, g_records = 0, g_fail_create_in = 0, g_fail_record_in = 0;
static float g_now = 0.0f;
static std::vector<StubEvent*> g_log;                              // every record, in order: a test completes events through it
static bool countdown(int& n) { return n > 0 && --n == 0; }       // true on the n-th call after it was armed
static hipError_t hipEventCreate(hipEvent_t* e) { if (countdown(g_fail_create_in)) return hipErrorOutOfMemory; *e = new StubEvent; ++g_created; return hipSuccess; }
static hipError_t hipEventDestroy(hipEvent_t e) { delete e; ++g_destroyed; return hipSuccess; }
static hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
  if (countdown(g_fail_record_in)) return hipErrorInvalidHandle;
  e->recorded = true; e->done = false; e->at = (g_now += 1.0f); e->stream = s; ++g_records; g_log.push_back(e);
  return hipSuccess;
}
static hipError_t hipEventQuery(hipEvent_t e) { return !e->recorded ? hipErrorInvalidHandle : e->done ? hipSuccess : hipErrorNotReady; }
static hipError_t hipEventSynchronize(hipEvent_t e) { if (!e->recorded) return hipErrorInvalidHandle; e->done = true; return hipSuccess; }
static hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) {
  if (!a->recorded || !b->recorded) return hipErrorInvalidHandle;
  *ms = b->at - a->at;
  return hipSuccess;
}
static hipError_t hipGetLastError() { return hipSuccess; }

#include "../ada-ray-tracer_amd/csrc/art_event_pairs.h"

using art::EventPairs;
#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x); std::exit(1); } } while (0)

struct Seen { std::vector<float> ms; std::vector<int> tag; };
static hipError_t fold(EventPairs& p, bool wait, Seen& s) { return p.fold(wait, [&s](float ms, uint8_t tag) { s.ms.push_back(ms); s.tag.push_back(tag); }); }
static void begin_end(EventPairs& p, hipStream_t s, uint8_t tag) {
  EventPairs::Timer t;
  CHECK(p.begin(t, s, tag) == hipSuccess);
  const int before = g_records;
  CHECK(t.end() == hipSuccess && g_records == before + 1);
  CHECK(t.end() == hipSuccess && g_records == before + 1);       // ending twice records once
}

int main() {
  int stream_a = 0, stream_b = 0;
  {                                                                // reuse: a steady state creates nothing
    EventPairs p;
    for (int round = 0; round < 3; ++round) {
      for (int k = 0; k < 3; ++k) begin_end(p, &stream_a, (uint8_t)(k | (round << 6)));
      CHECK(p.live() == 3 && g_created == 6);
      Seen s;
      CHECK(fold(p, true, s) == hipSuccess && s.ms.size() == 3 && p.live() == 0 && p.idle() == 3);
      for (int k = 0; k < 3; ++k) CHECK(s.ms[(size_t)k] == 1.0f && (s.tag[(size_t)k] & 15) == k && (s.tag[(size_t)k] >> 6) == round);      // the pairs of this round, not stale ones
    }
    p.destroy();
    CHECK(g_destroyed == 6 && p.idle() == 0);
  }
  {                                                                // rollback: a pair without a first record never becomes live
    EventPairs p;
    g_fail_create_in = 2;                                          // the second event cannot be created: the first one is given back
    { EventPairs::Timer t; CHECK(p.begin(t, &stream_a) == hipErrorOutOfMemory); }
    CHECK(p.live() == 0 && p.idle() == 0 && g_created - g_destroyed == 0);
    g_fail_record_in = 1;
    const int before = g_records;
    { EventPairs::Timer t; CHECK(p.begin(t, &stream_a) == hipErrorInvalidHandle); CHECK(t.end() == hipSuccess); }      // ... and its timer records nothing
    CHECK(p.live() == 0 && p.idle() == 1 && g_records == before);
    begin_end(p, &stream_a, 0);                                    // the pair is reused
    CHECK(p.live() == 1 && p.idle() == 0 && g_created - g_destroyed == 2);
    p.destroy();
  }
  {                                                                // the timer ends on every way out, on begin()'s stream; cancel takes a pair out
    EventPairs p;
    { EventPairs::Timer t; CHECK(p.begin(t, &stream_b, 7) == hipSuccess); }
    Seen s;
    CHECK(fold(p, true, s) == hipSuccess && s.ms.size() == 1 && s.tag[0] == 7);
    begin_end(p, &stream_a, 1);
    const int before = g_records;
    { EventPairs::Timer t; CHECK(p.begin(t, &stream_a, 2) == hipSuccess); begin_end(p, &stream_a, 3); t.cancel(); t.cancel(); }      // (not the newest pair)
    CHECK(g_records == before + 3 && p.live() == 2 && p.idle() == 1);      // the cancelled pair's second event was not recorded
    { EventPairs::Timer t; CHECK(p.begin(t, &stream_a, 4) == hipSuccess); CHECK(t.end() == hipSuccess); t.cancel(); }      // cancel after end: still counted
    s = Seen();
    CHECK(fold(p, true, s) == hipSuccess && s.tag.size() == 3 && s.tag[0] == 1 && s.tag[1] == 3 && s.tag[2] == 4);
    p.destroy();
  }
  {                                                                // a querying fold keeps what is in flight; release drops it
    EventPairs p;
    g_log.clear();
    for (int k = 0; k < 3; ++k) {
      EventPairs::Timer t;
      CHECK(p.begin(t, &stream_a, (uint8_t)k) == hipSuccess);
    }
    Seen s;
    CHECK(fold(p, false, s) == hipSuccess && s.ms.empty() && p.live() == 3);      // (a stub event completes when somebody waits for it, or a test says so)
    CHECK(g_log.size() == 6 && g_log[1]->stream == &stream_a);
    g_log[1]->done = g_log[5]->done = true;                        // the first and the third pair have completed
    CHECK(fold(p, false, s) == hipSuccess && s.tag.size() == 2 && s.tag[0] == 0 && s.tag[1] == 2 && p.live() == 1 && p.idle() == 2);
    CHECK(fold(p, false, s) == hipSuccess && s.tag.size() == 2 && p.live() == 1);
    g_log[3]->done = true;
    CHECK(fold(p, false, s) == hipSuccess && s.tag.size() == 3 && s.tag[2] == 1 && p.live() == 0 && p.idle() == 3);
    begin_end(p, &stream_a, 9);
    p.release();
    CHECK(p.live() == 0 && p.idle() == 3);
    s = Seen();
    CHECK(fold(p, true, s) == hipSuccess && s.ms.empty());
    p.destroy();
  }
  {                                                                // a waiting fold: the first error once, that pair and the later ones stay
    EventPairs p;
    begin_end(p, &stream_a, 0);
    { EventPairs::Timer t; CHECK(p.begin(t, &stream_a, 1) == hipSuccess); g_fail_record_in = 1; CHECK(t.end() == hipErrorInvalidHandle); }      // second event never recorded
    begin_end(p, &stream_a, 2);
    Seen s;
    CHECK(fold(p, true, s) == hipErrorInvalidHandle && s.tag.size() == 1 && s.tag[0] == 0 && p.live() == 2 && p.idle() == 1);
    s = Seen();
    g_log.back()->done = true;                                     // (the last pair's second event: the waiting fold stopped before it)
    CHECK(fold(p, false, s) == hipSuccess && s.tag.size() == 1 && s.tag[0] == 2 && p.live() == 1);      // a querying fold reports nothing and goes on
    p.destroy();
  }
  CHECK(g_created == g_destroyed);
  std::printf("event pairs ok: %d events created and destroyed, %d records\n", g_created, g_records);
  return 0;
}
