// stream.hip -- host-only: the launch path (stream.h).  Tail events and their learned per-call plan, the one cross-stream wait,
// the side stream with its forks, joins and gradient-segment events, the weight-gradient routing, the scope of a C-ABI call,
// and the profiling rings whose brackets ride on the same launches.
#include "stream.h"
#include "kernels.h"

#include <stdarg.h>

// ---- tail events (stream.h) ----
namespace {
constexpr int kTailRing = 64, kTailStreams = 8, kPlanWords = 8, kPlans = 32;   // (a plan covers 64 * kPlanWords launches per stream)
hipStream_t const kDepMany = reinterpret_cast<hipStream_t>(~(uintptr_t)0);
struct TailTrack {
  bool used = false;
  hipStream_t s = nullptr;
  hipEvent_t ring[kTailRing] = {};
  int next = 0;
  int tail_slot = -1;          // ring slot that still owns `tail` (-1: stolen, not a ring event, or no tail)
  hipEvent_t tail = nullptr;   // rides on the last launch on s; nullptr once anything it does not cover was enqueued behind it
  bool has_dep = false;        // behind the last launch s was made to wait for events of stream `dep` (kDepMany: of several streams):
  hipStream_t dep = nullptr;   //   `tail` then still covers everything a fork TO `dep` has to wait for (dep's own order covers the rest)
  int launches = 0;            // launches on s in this scope
  int tail_idx = -1;           // launch index of `tail`
  bool declined = false;       // the last launch on s carried no event because the plan did not ask for one
  int dev = 0;                 // device the ring's events belong to
  uint64_t stamp = 0;          // last use (least-recently-used take-over when a caller keeps handing in new streams)
  bool armed = false;          // profiling bracket: the next launch carries these two events
  hipEvent_t arm_start = nullptr, arm_stop = nullptr;
  int arm_launches = 0;
};
// Which launches of a call need an event is learned, not declared: the first call of a kind / shape puts an event on EVERY launch
// and notes the (stream, launch index) pairs a fork, join or segment actually consumed; later calls put events on those only
// (an event on all ~90 launches of a step costs what the ~17 markers it replaces cost: measured, profiles/r06_tail_events_ab.txt).
// A fork that finds no event because the plan declined it falls back to a recorded marker -- always correct -- and the plan is
// learned again by the next call.
struct TailPlan {
  bool used = false, learned = false;
  uint64_t key = 0;
  uint64_t bits[kTailStreams][kPlanWords] = {};
};
thread_local TailTrack g_tail[kTailStreams];
thread_local TailPlan g_plans[kPlans];
thread_local TailPlan* g_plan = nullptr;
thread_local int g_plan_next = 0;
thread_local bool g_tail_on = false, g_learning = false;
thread_local uint64_t g_tail_clock = 0;
void tail_drop(TailTrack* t);
TailTrack* tail_find(hipStream_t s, bool create) {
  for (TailTrack& t : g_tail)
    if (t.used && t.s == s) {
      t.stamp = ++g_tail_clock;
      return &t;
    }
  if (!create) return nullptr;
  int dev = 0;
  (void)hipGetDevice(&dev);
  TailTrack* lru = nullptr;
  for (TailTrack& t : g_tail) {
    if (!t.used) {
      t.used = true;
      t.s = s;
      t.dev = dev;
      t.stamp = ++g_tail_clock;
      return &t;
    }
    // a caller that hands in ever new streams: the least recently used entry of the SAME device is taken over (its ring events
    // are not bound to a stream); entries of streams that launched in this scope are left alone
    if (t.dev == dev && t.launches == 0 && !t.tail && !t.armed && (!lru || t.stamp < lru->stamp)) lru = &t;
  }
  if (lru) {
    lru->s = s;
    lru->stamp = ++g_tail_clock;
    tail_drop(lru);
    lru->tail_idx = -1;
    lru->declined = false;
  }
  return lru;
}
void tail_consumed(TailTrack* t) {
  if (g_learning && g_plan && t->tail_idx >= 0 && t->tail_idx < 64 * kPlanWords)
    g_plan->bits[t - g_tail][t->tail_idx >> 6] |= 1ull << (t->tail_idx & 63);
}
void tail_drop(TailTrack* t) {
  t->tail = nullptr;
  t->tail_slot = -1;
  t->has_dep = false;
  t->dep = nullptr;
}

// the event of the LAST launch on s if it covers everything `for_stream` has to wait for, else nullptr
hipEvent_t tail_event(hipStream_t s, hipStream_t for_stream) {
  if (!g_tail_on) return nullptr;
  TailTrack* t = tail_find(s, false);
  if (!t) return nullptr;
  if (t->tail && t->has_dep && (t->dep == kDepMany || t->dep != for_stream)) return nullptr;   // (waits behind the launch that `for_stream` does not inherit by its own order)
  if (t->tail) tail_consumed(t);
  else if (t->declined && g_plan && !g_learning) g_plan->learned = false;   // (mispredicted: this call falls back, the next one learns)
  return t->tail;
}
// tail event for a longer-lived use: taken OUT of the ring (*owned; `give` refills the slot) or an alias of an event the ring does not own; nullptr: none
hipEvent_t tail_steal(hipStream_t s, hipEvent_t give, bool* owned) {
  *owned = false;
  hipEvent_t e = tail_event(s, nullptr);
  if (!e) return nullptr;
  TailTrack* t = tail_find(s, false);
  if (t->tail_slot >= 0 && t->ring[t->tail_slot] == e) {
    t->ring[t->tail_slot] = give;   // (an event lives in exactly one place: a ring slot or its new owner)
    t->tail_slot = -1;
    *owned = true;
  }
  return e;   // (not owned: a profiling bracket's stop event, or one that was stolen before -- whoever waits for it does so before it is bound again)
}
// something that is not a library launch was enqueued on s
void tail_touch(hipStream_t s) {
  TailTrack* t = tail_find(s, false);
  if (t) {
    tail_drop(t);
    t->declined = false;
  }
}
// opens the scope of one C-ABI call; key = kind + shape of the call (its launch plan)
void tail_open(uint64_t key) {
  const int mode = sw_int<SW_TAIL_EVENTS>();
  g_tail_on = mode != 0;
  g_plan = nullptr;
  g_learning = false;
  for (TailTrack& t : g_tail) {
    tail_drop(&t);
    t.launches = 0;
    t.tail_idx = -1;
    t.declined = false;
    t.armed = false;
  }
  if (!g_tail_on) return;
  for (TailPlan& p : g_plans)
    if (p.used && p.key == key) g_plan = &p;
  if (!g_plan) {
    g_plan = &g_plans[g_plan_next];
    g_plan_next = (g_plan_next + 1) % kPlans;
    *g_plan = TailPlan();
    g_plan->used = true;
    g_plan->key = key;
  }
  if (!g_plan->learned || mode == 2) {   // (TACO_TAIL_EVENTS=2: an event on every launch, always)
    g_learning = true;
    for (auto& row : g_plan->bits)
      for (uint64_t& w : row) w = 0;
  }
}
void tail_close() {
  if (g_tail_on && g_learning && g_plan) g_plan->learned = true;
  g_tail_on = false;
  g_learning = false;
  g_plan = nullptr;
  for (TailTrack& t : g_tail) {
    tail_drop(&t);
    t.armed = false;
  }
}
// profiling ring: inside a scope a bracket's start / stop events ride on the bracketed launch itself instead of two markers
bool tail_arm_timing(hipStream_t s, hipEvent_t start, hipEvent_t stop) {   // false: no scope, the caller records `start`
  if (!g_tail_on) return false;
  TailTrack* t = tail_find(s, true);
  if (!t) return false;
  t->armed = true;
  t->arm_start = start;
  t->arm_stop = stop;
  t->arm_launches = 0;
  return true;
}
int tail_disarm_timing(hipStream_t s) {   // launches on s since the arm (1: the pair rode on that launch; else the caller records what is missing)
  TailTrack* t = tail_find(s, false);
  if (!t) return 0;
  t->armed = false;
  return t->arm_launches;
}
}  // namespace

hipEvent_t taco_tail_take(hipStream_t s, hipEvent_t* start) {
  *start = nullptr;
  if (!g_tail_on) return nullptr;
  TailTrack* t = tail_find(s, true);
  if (!t) return nullptr;   // (more streams than the table holds: those launch plainly and fork through recorded events)
  const int idx = t->launches++;
  ++t->arm_launches;
  t->has_dep = false;       // (this launch is ordered behind every wait enqueued so far: its event covers them)
  t->dep = nullptr;
  if (t->armed) {           // a profiling bracket's pair: timing events the ring does not own
    t->armed = false;
    *start = t->arm_start;
    t->tail = t->arm_stop;
    t->tail_slot = -1;
    t->tail_idx = idx;
    t->declined = false;
    return t->tail;
  }
  const bool want = g_learning || (g_plan && idx < 64 * kPlanWords && ((g_plan->bits[t - g_tail][idx >> 6] >> (idx & 63)) & 1));
  if (!want) {
    tail_drop(t);
    t->declined = true;
    return nullptr;
  }
  const int slot = t->next;
  t->next = (slot + 1) % kTailRing;
  t->declined = false;
  if (!t->ring[slot] && hipEventCreateWithFlags(&t->ring[slot], hipEventDisableTiming) != hipSuccess) {
    t->ring[slot] = nullptr;
    tail_drop(t);
    return nullptr;
  }
  t->tail = t->ring[slot];
  t->tail_slot = slot;
  t->tail_idx = idx;
  return t->tail;
}

int taco_memset_async(void* p, int v, size_t bytes, hipStream_t s, const char* what) {
  const hipError_t e = hipMemsetAsync(p, v, bytes, s);
  tail_touch(s);
  if (e != hipSuccess) {
    taco_set_error("%s: memset: %s", what, hipGetErrorString(e));
    return TACO_ELAUNCH;
  }
  return TACO_OK;
}
int taco_upload_async(void* dst, const void* host_src, size_t bytes, hipStream_t s, const char* what) {
  const hipError_t e = hipMemcpyAsync(dst, host_src, bytes, hipMemcpyHostToDevice, s);
  tail_touch(s);
  if (e != hipSuccess) {
    taco_set_error("%s: %s", what, hipGetErrorString(e));
    return TACO_ELAUNCH;
  }
  return TACO_OK;
}

// ---- the cross-stream wait ----
static hipEvent_t record_fallback(hipStream_t producer, hipEvent_t* fallback) {
  if (!fallback) return nullptr;
  if (!*fallback && hipEventCreateWithFlags(fallback, hipEventDisableTiming) != hipSuccess) *fallback = nullptr;
  return *fallback && hipEventRecord(*fallback, producer) == hipSuccess ? *fallback : nullptr;
}
StreamMark stream_mark(hipStream_t producer, hipStream_t waiter, hipEvent_t* fallback) {
  StreamMark m;
  m.producer = producer;
  m.fallback = fallback;
  m.ev = tail_event(producer, waiter);
  m.tail = m.ev != nullptr;
  if (!m.ev) m.ev = record_fallback(producer, fallback);
  return m;
}
int stream_wait_mark(hipStream_t waiter, StreamMark m) {
  if (m.tail) {
    if (hipStreamWaitEvent(waiter, m.ev, 0) == hipSuccess) {
      // the wait itself is not covered by the waiter's last launch -- except for a fork back TO the producer, whose own order
      // covers it (m.ev lies in the producer's past, however long ago the mark was taken)
      if (TailTrack* w = tail_find(waiter, false)) {
        if (!w->has_dep) {
          w->has_dep = true;
          w->dep = m.producer;
        } else if (w->dep != m.producer) {
          w->dep = kDepMany;
        }
      }
      return TACO_OK;
    }
    (void)hipGetLastError();
    m.ev = record_fallback(m.producer, m.fallback);   // (the tail event cannot be waited for: a recorded one, of the producer as it is now)
  }
  if (!m.ev || hipStreamWaitEvent(waiter, m.ev, 0) != hipSuccess) return TACO_ELAUNCH;
  tail_touch(waiter);
  return TACO_OK;
}
int stream_wait(hipStream_t waiter, hipStream_t producer, hipEvent_t* fallback) {
  return stream_wait_mark(waiter, stream_mark(producer, waiter, fallback));
}

// ---- HIP-event profiling rings (taco_profile_enable / taco_profile_read[2]) ----
// category: 0 decoder forward kernel, 1 decoder backward kernel, 2 MFMA GEMM family (conv_gemm, gemm_tn, highway stack),
// 3 bi-GRU recurrences.  Every bracketed launch gets a hipEventRecord pair on ITS launch stream plus its algorithmic FLOPs.
namespace {
struct ProfRing {
  static constexpr int kCap = 4096;
  hipEvent_t start[kCap], stop[kCap];
  double flops[kCap];
  bool armed[kCap];       // the pair rides on the bracketed launch (tail events) instead of being recorded as two markers
  char label[kCap][96];   // what the launch was (taco_prof_label; read by taco_debug_profile_labels before taco_profile_read2)
  int created = 0;   // events created so far (lazily, in steps: creating 2 x 4096 events up front costs milliseconds)
  int n = 0;
};
ProfRing g_prof[4];
int g_prof_mask = 0;   // bit c: category c is recorded
}  // namespace

int taco_prof_begin(int which, hipStream_t s) {
  if (!(g_prof_mask & (1 << which))) return -1;
  ProfRing& r = g_prof[which];
  if (r.n >= ProfRing::kCap) return -1;
  while (r.created <= r.n) {
    if (hipEventCreate(&r.start[r.created]) != hipSuccess || hipEventCreate(&r.stop[r.created]) != hipSuccess) return -1;
    ++r.created;
  }
  // inside a tail-event scope the pair rides on the bracketed launch itself -- two marker packets around the decoder
  // kernels were ~20 us of the timed step; outside (op-level calls, capture) the bracket is two recorded markers as before
  r.armed[r.n] = tail_arm_timing(s, r.start[r.n], r.stop[r.n]);
  if (!r.armed[r.n]) (void)hipEventRecord(r.start[r.n], s);
  r.label[r.n][0] = 0;
  return r.n;
}
void taco_prof_label(int which, int slot, const char* fmt, ...) {
  if (slot < 0) return;
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_prof[which].label[slot], sizeof(g_prof[which].label[slot]), fmt, ap);
  va_end(ap);
}
void taco_prof_end(int which, int slot, hipStream_t s, double flops) {
  if (slot < 0) return;
  ProfRing& r = g_prof[which];
  if (!r.armed[slot]) {
    (void)hipEventRecord(r.stop[slot], s);
  } else {
    // the pair was armed for the next launch on s.  One launch since: it carried both events.  Several (a k-split pair, the decoder
    // in chunks of 32 rows): the first one carried both -- `stop` is recorded again behind the last, which is what counts.  None:
    // both are recorded now.
    const int rode = tail_disarm_timing(s);
    if (rode == 0) (void)hipEventRecord(r.start[slot], s);
    if (rode != 1) (void)hipEventRecord(r.stop[slot], s);
  }
  r.flops[slot] = flops;
  r.n = slot + 1;
}
void taco_prof_cancel(int which, int slot, hipStream_t s) {
  // (the ring does not advance: the next bracket reuses the slot; an unarmed bracket's recorded start is simply overwritten)
  if (slot >= 0 && g_prof[which].armed[slot]) (void)tail_disarm_timing(s);
}
extern "C" int taco_profile_enable(int mask) {
  g_prof_mask = mask & 31;
  return TACO_OK;
}
extern "C" int taco_profile_read2(int which, float* ms, double* flops, int cap) {
  TACO_REQUIRE(which >= 0 && which < 4, "profile_read: category %d out of range", which);
  ProfRing& r = g_prof[which];
  int n = 0;
  for (int i = 0; i < r.n; ++i) {
    if (hipEventSynchronize(r.stop[i]) != hipSuccess) break;
    float t = 0.f;
    if (hipEventElapsedTime(&t, r.start[i], r.stop[i]) != hipSuccess) break;
    if (ms && n < cap) ms[n] = t;
    if (flops && n < cap) flops[n] = r.flops[i];
    ++n;
  }
  r.n = 0;
  return n;
}
extern "C" int taco_profile_read(int which, float* ms, int cap) { return taco_profile_read2(which, ms, nullptr, cap); }
extern "C" int taco_debug_profile_labels(int which, char* buf, int cap) {
  TACO_REQUIRE(which >= 0 && which < 4 && buf && cap > 0, "profile_labels: bad arguments");
  ProfRing& r = g_prof[which];
  int pos = 0;
  for (int i = 0; i < r.n; ++i) {
    const int w = snprintf(buf + pos, cap - pos, "%s\n", r.label[i]);
    if (w < 0 || pos + w >= cap) break;
    pos += w;
  }
  buf[pos < cap ? pos : cap - 1] = 0;
  return r.n;
}

// ---- side stream (stream.h) ----
namespace {
struct SideStream {
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;   // what a fork / join records when the producer has no tail event
  hipEvent_t ev_img = nullptr;   // the forward weight images are built (recorded on the side stream; the main stream waits in front of the encoder CBHG)
  bool off = false;
  hipEvent_t ev_seg[kGradSegments] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev_seg_use[kGradSegments] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // what wait_grad_segment waits for: ev_seg or a tail event
  bool seg_recorded = false;
};
SideStream& side_stream() {
  static thread_local SideStream ss[16];
  int dev = 0;
  (void)hipGetDevice(&dev);
  SideStream& x = ss[dev & 15];
  if (!x.side && !x.off) {
    if (sw_on<SW_NO_OVERLAP>() || hipStreamCreateWithFlags(&x.side, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&x.ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&x.ev_join, hipEventDisableTiming) != hipSuccess) {
      x.side = nullptr;
      x.off = true;
    }
  }
  return x;
}
}  // namespace

hipStream_t side_stream_or_null() { return side_stream().side; }
hipStream_t side_fork(hipStream_t s) {
  SideStream& x = side_stream();
  // (profile bit 4: everything on the caller's stream, so that the per-launch event timing of the GEMM family measures each
  //  kernel by itself instead of two streams' kernels sharing the chip)
  if (x.off || (g_prof_mask & 16)) return s;
  return stream_wait(x.side, s, &x.ev_fork) == TACO_OK ? x.side : s;
}
int side_join(hipStream_t s, hipStream_t side) {
  if (side == s) return TACO_OK;
  if (stream_wait(s, side, &side_stream().ev_join) != TACO_OK) {
    taco_set_error("side_join: event record/wait failed");
    return TACO_ELAUNCH;
  }
  return TACO_OK;
}
StreamMark side_mark_images(hipStream_t side, hipStream_t s) {
  // (tail events: the image launch's own event.  Its ring slot comes round again after 64 more launches on the side stream --
  //  far more than are enqueued before the wait -- and would then name a LATER launch of the same stream: still correct)
  return stream_mark(side, s, &side_stream().ev_img);
}
int record_segment(int seg, hipStream_t on) {
  SideStream& x = side_stream();
  if (!x.ev_seg[seg] && hipEventCreateWithFlags(&x.ev_seg[seg], hipEventDisableTiming) != hipSuccess) {
    taco_set_error("taco_backward: cannot create the gradient-segment event");
    return TACO_ELAUNCH;
  }
  // (tail events: the segment's event is the one riding on the last launch on `on` -- taken out of that stream's ring, this
  //  segment's previous event refills the slot -- instead of a marker behind it)
  bool owned = false;
  if (hipEvent_t t = tail_steal(on, x.ev_seg[seg], &owned)) {
    if (owned) x.ev_seg[seg] = t;
    x.ev_seg_use[seg] = t;   // (not owned: the stop event of a profiling bracket -- wait_grad_segment waits for it before it is bound again)
  } else {
    // no tail event to take (`on` waits for side-stream work behind its last launch: the end of the pass): the marker goes to the
    // SIDE stream, made to wait for `on`'s last launch first -- it covers both streams and sits between no two kernels of `on`
    hipStream_t at = on;
    if (x.side && x.side != on && !x.off && stream_wait(x.side, on, nullptr) == TACO_OK) at = x.side;
    if (hipEventRecord(x.ev_seg[seg], at) != hipSuccess) {
      taco_set_error("taco_backward: hipEventRecord(segment %d) failed", seg);
      return TACO_ELAUNCH;
    }
    x.ev_seg_use[seg] = x.ev_seg[seg];
  }
  if (seg == 0) x.seg_recorded = true;
  return TACO_OK;
}
int wait_grad_segment(int seg, hipStream_t stream) {
  SideStream& x = side_stream();
  TACO_REQUIRE(x.seg_recorded && x.ev_seg_use[seg], "taco_wait_grad_segment: no taco_backward was issued by this thread on this device");
  if (hipStreamWaitEvent(stream, x.ev_seg_use[seg], 0) != hipSuccess) {
    taco_set_error("taco_wait_grad_segment: hipStreamWaitEvent failed");
    return TACO_ELAUNCH;
  }
  return TACO_OK;
}

// ---- weight-gradient routing (stream.h) ----
static thread_local hipStream_t g_tn_side = nullptr;
static thread_local hipEvent_t g_tn_ev = nullptr;
ScopedRoute::ScopedRoute(hipStream_t side) : prev(g_tn_side) { g_tn_side = side; }
ScopedRoute::~ScopedRoute() { g_tn_side = prev; }
int tn_route(hipStream_t s, hipStream_t* out) {
  *out = s;
  if (!g_tn_side || g_tn_side == s || (g_prof_mask & 16)) return TACO_OK;
  if (!g_tn_ev && hipEventCreateWithFlags(&g_tn_ev, hipEventDisableTiming) != hipSuccess) {
    taco_set_error("weight-gradient side stream: cannot create an event");
    return TACO_ELAUNCH;
  }
  if (stream_wait(g_tn_side, s, &g_tn_ev) != TACO_OK) {
    taco_set_error("weight-gradient side stream: event record/wait failed");
    return TACO_ELAUNCH;
  }
  *out = g_tn_side;
  return TACO_OK;
}

CallScope::CallScope(hipStream_t s, int kind, const TacoShape& sh) {
  weight_images_clear();
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &st) != hipSuccess) {
    (void)hipGetLastError();   // (not this call's failure to report: launches are checked with hipGetLastError)
    return;
  }
  if (st != hipStreamCaptureStatusNone) return;
  uint64_t key = 1469598103934665603ull;   // (FNV-1a over the call's kind and shape)
  const int64_t f[8] = {kind, sh.B, sh.Tt, sh.Td, sh.r, sh.V, sh.S, (int64_t)(uintptr_t)s};
  for (int64_t v : f) key = (key ^ (uint64_t)v) * 1099511628211ull;
  tail_open(key);
  tails = true;
}
CallScope::~CallScope() {
  if (tails) tail_close();
  weight_images_clear();
  g_tn_side = nullptr;
  tn_queue_reset();
}
