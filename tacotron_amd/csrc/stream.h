// stream.h -- the launch path: how a kernel is launched, how one stream waits for another, and the per-call host state
// around both (stream.hip).  Everything here only ENQUEUES; a mistake in this file's callers is a race, not a crash.
#pragma once
#include "common.h"

// ---- tail events: cross-stream dependencies without marker packets -----------------------------------------------------
// A fork / join between two streams used to be hipEventRecord on the producing stream + hipStreamWaitEvent on the consuming one.
// The record is a marker packet with a system-scope release BETWEEN two kernels of the producing stream: 7-12 us of bubble per
// fork in the step's timeline (~17 of them on the critical path), 4.6 us with empty kernels in tools/micro/event_gap.hip
// (profiles/r06_event_gap.txt: record + wait 6.5 us per kernel vs 1.9 plain; hipExtLaunchKernelGGL's stop event + wait 3.0).
// While a CallScope is open (taco_forward / taco_backward / taco_infer; not while the stream is being captured), every launch
// of the library carries a stop event of a per-stream ring on its OWN dispatch packet; "everything enqueued on s so far" is then
// the event of the last kernel launched on s (streams are in order), and a fork / join waits for that -- no marker.  Whatever
// else is enqueued on a stream (memset, copy, event wait) "touches" it: its tail event no longer covers the stream and the next
// fork falls back to a recorded event.  That is why every such enqueue goes through a function of this file.
// TACO_TAIL_EVENTS=0: recorded events everywhere (A/B runs).
hipEvent_t taco_tail_take(hipStream_t s, hipEvent_t* start);   // the stop event the NEXT launch on s carries (nullptr: none) and, for a launch bracketed by the profiling ring, its start event

#define TACO_KLAUNCH(kernel, grid, block, smem, stream, ...)                                                        \
  do {                                                                                                              \
    hipEvent_t tst__ = nullptr;                                                                                     \
    hipEvent_t tev__ = taco_tail_take(stream, &tst__);                                                              \
    if (tev__) hipExtLaunchKernelGGL(kernel, grid, block, smem, stream, tst__, tev__, 0, __VA_ARGS__);              \
    else hipLaunchKernelGGL(kernel, grid, block, smem, stream, __VA_ARGS__);                                        \
  } while (0)

// What is enqueued on a stream and is not a kernel: the call, the touch, and on failure TACO_ELAUNCH with the error string
// "<what>: memset: <HIP error>" / "<what>: <HIP error>".
int taco_memset_async(void* p, int v, size_t bytes, hipStream_t s, const char* what);
int taco_upload_async(void* dst, const void* host_src, size_t bytes, hipStream_t s, const char* what);

// `waiter` waits for everything enqueued on `producer` so far: for the producer's tail event if it has one that covers the
// stream, else for *fallback (created on first use), recorded on the producer now.  fallback == nullptr: the tail event or
// nothing.  TACO_OK, or TACO_ELAUNCH with nothing enqueued on the waiter (the error string is the caller's to set).
// The two halves, for a wait that is enqueued later than the point it covers: stream_mark() names that point, stream_wait_mark()
// waits for it; stream_wait() is one behind the other.  If the wait for a mark's tail event fails, *fallback is recorded then:
// the waiter waits for the producer as it is at the wait, a superset.  `fallback` must outlive the mark.
struct StreamMark {
  hipEvent_t ev = nullptr;     // nullptr: no event could be had
  bool tail = false;           // ev rides on the producer's last launch (else: *fallback, recorded)
  hipStream_t producer = nullptr;
  hipEvent_t* fallback = nullptr;
};
StreamMark stream_mark(hipStream_t producer, hipStream_t waiter, hipEvent_t* fallback);
int stream_wait_mark(hipStream_t waiter, StreamMark m);
int stream_wait(hipStream_t waiter, hipStream_t producer, hipEvent_t* fallback);

// ---- side stream -------------------------------------------------------------------------------------------------------
// Work that is independent of the main chain runs here while a 64-workgroup recurrent kernel (bi-GRU) or the encoder leaves
// most of the chip idle.  side_fork(): the side stream waits for everything enqueued on `s` so far (returns `s` itself when
// there is no side stream); side_join(): `s` waits for the side work.  No host synchronisation; TACO_NO_OVERLAP=1 keeps
// everything on `s`.
hipStream_t side_stream_or_null();   // this thread's side stream on the current device
hipStream_t side_fork(hipStream_t s);
int side_join(hipStream_t s, hipStream_t side);
StreamMark side_mark_images(hipStream_t side, hipStream_t s);   // the forward weight images are built: everything on `side` so far, for `s` to wait for

// Gradient-segment events of the most recent taco_backward issued by this thread on this device: segment [4] post-net,
// [3] decoder, [2] encoder projections / highways / bi-GRU, [1] encoder conv bank, [0] embedding + encoder pre_net of the flat
// gradient buffer is final.
constexpr int kGradSegments = 5;
int record_segment(int seg, hipStream_t on);
int wait_grad_segment(int seg, hipStream_t stream);

// ---- weight-gradient routing -------------------------------------------------------------------------------------------
// While a ScopedRoute is alive, every weight-gradient launch issued for stream `s` goes to that stream instead, ordered behind the
// work enqueued on `s` so far.  The CBHG backward passes use it: their ~27 weight-gradient GEMMs (0.5 / 0.7 ms per step) feed
// nothing but the gradient buffer, so they run beside the activation-gradient chain -- much of which is small launches that
// leave most CUs idle -- instead of inside it.  Their operands then must not be reused in place by the chain
// (BwdScratch::alt_*).  TACO_NO_SIDE_TN=1 keeps them on the main stream (A/B runs).
int tn_route(hipStream_t s, hipStream_t* out);   // *out: the stream a weight gradient issued for `s` launches on
void tn_queue_reset();                           // (model.hip: empties the queue of grouped weight-gradient launches)

// Installs `side` (nullptr: none) as this thread's weight-gradient route for one stretch of code and puts the previous route back
// when the stretch ends, on every return path.
struct ScopedRoute {
  const hipStream_t prev;
  explicit ScopedRoute(hipStream_t side);
  ScopedRoute(const ScopedRoute&) = delete;
  ~ScopedRoute();
};

// The scope of one model-level C-ABI call (taco_forward / taco_infer / taco_backward), constructed first, after argument
// validation.  Host state the call installs on this thread dies with it, on every return path: the weight-image table (keyed by
// this call's parameter pointers, pointing into its workspace) is emptied on entry and on exit, and the weight-gradient routing
// and the TN queue are left empty.  Tail events are tracked while the scope is alive -- not while the caller's stream is being
// captured into a graph (a stop event on a captured launch is not a graph dependency).
struct CallScope {
  bool tails = false;
  CallScope(hipStream_t s, int kind, const TacoShape& sh);   // kind + shape + stream: the key of the call's launch plan
  ~CallScope();
};

// ---- profiling rings (taco_profile_enable / taco_profile_read[2]) ------------------------------------------------------
// category 0 / 1: decoder fwd / bwd kernel, 2: MFMA GEMM family, 3: bi-GRU recurrences.  begin returns a slot (or -1 when the
// category is not being recorded); end stamps the stop event and the launch's algorithmic FLOPs.
int taco_prof_begin(int which, hipStream_t s);
void taco_prof_end(int which, int slot, hipStream_t s, double flops);
void taco_prof_cancel(int which, int slot, hipStream_t s);   // the bracketed launch was not made: drops the slot, records nothing
void taco_prof_label(int which, int slot, const char* fmt, ...) __attribute__((format(printf, 3, 4)));   // no-op when slot < 0
