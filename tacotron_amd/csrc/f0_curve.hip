// f0_curve.hip -- the intonation range of an utterance (include/taco_hip.h taco_f0_range_curve): a tracked pitch contour turned into
// the per-frame step curve taco_frames_pitch_curve consumes, every frame's distance from the row's own level, in octaves, scaled
// by k.  No counterpart in the reference.  One launch, one workgroup of 256 threads per row, everything of the row in LDS:
//
// (a) Centre.  f0_row_stats of frames.h, the two-pass fixed tree of taco_f0_stats: the count, the centre c and the deviation have
// that call's bits.  A row at the neutral scale, or without a voiced frame, copies clamp(base) (or TACO_PITCH_ONE) and ends here:
// no logarithm, no exponential.
// (b) Deviations and ballots.  Thread t takes the frames t, t + 256, ...: d[f] = log2f(period) - c of a voiced frame goes to LDS
// (32 KiB at the cap of 8192 frames), and a wave's 64 voiced flags are one ballot, one 64-bit word per 64 frames (128 words at the
// cap).
// (c) Neighbours, in integers.  Word w learns the last voiced frame in front of it and the first one behind it by walking the
// words (one thread per word; the walk ends at the first word with a bit, so it is as long as the row's longest gap); inside a
// word the nearest voiced frame below / above a bit is a count of leading / trailing zeros of the masked word, as phase_init.hip
// finds its lobe owners.  An unvoiced frame between two voiced ones is their straight line, one with a single neighbour holds it.
// The voiced entries of d are only read in this pass and the unvoiced ones only written, each by its own thread.
// (d) Smoothing, excursion, base and step per frame, in the order the header states.  Nothing is contracted in this file, so the
// float32 restatement of tests/f0_range_ref.py differs from the device by its log2 / exp2 alone.
// No atomics anywhere: the same arguments give the same bits.
#include "frames.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int kCurveWords = TACO_STRETCH_MAX_FRAMES / 64;
constexpr int kMaxScaleQ = 4 * 65536;

__device__ __forceinline__ int clamp_pitch_step(int s) {
  return s < TACO_PITCH_MIN_STEP ? TACO_PITCH_MIN_STEP : (s > TACO_PITCH_MAX_STEP ? TACO_PITCH_MAX_STEP : s);
}

__global__ __launch_bounds__(256) void f0_range_curve_kernel(const float* __restrict__ period, const int32_t* __restrict__ frames,
                                                             int frames_per_unit, const int32_t* __restrict__ scale_q,
                                                             const int32_t* __restrict__ base_q, int W, float limit,
                                                             int32_t* __restrict__ step_q, float* stats, int F) {
  __shared__ float red[256];
  __shared__ int cnt[256];
  __shared__ float d[TACO_STRETCH_MAX_FRAMES];
  __shared__ unsigned long long bal[kCurveWords];
  __shared__ int before[kCurveWords], after[kCurveWords];   // the nearest voiced frame outside word w on either side, -1: none
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Fb = row_frames_uniform(frames, frames_per_unit, b, F);
  const float* __restrict__ p = period + (int64_t)b * F;
  const int32_t* __restrict__ base = base_q ? base_q + (int64_t)b * F : nullptr;
  int32_t* __restrict__ out = step_q + (int64_t)b * F;
  const F0RowStats r = f0_row_stats(p, nullptr, Fb, tid, red, cnt);
  if (stats && tid == 0) {
    stats[3 * b] = (float)r.n;
    stats[3 * b + 1] = r.mean;
    stats[3 * b + 2] = r.n > 0 ? sqrtf(r.ss / (float)r.n) : 0.f;
  }
  for (int f = Fb + tid; f < F; f += 256) out[f] = TACO_PITCH_ONE;
  int kq = scale_q ? scale_q[b] : TACO_PITCH_ONE;
  kq = kq < 0 ? 0 : (kq > kMaxScaleQ ? kMaxScaleQ : kq);
  if (kq == TACO_PITCH_ONE || r.n == 0) {   // (the same decision in every thread: both come from one address each)
    for (int f = tid; f < Fb; f += 256) out[f] = base ? clamp_pitch_step(base[f]) : TACO_PITCH_ONE;
    return;
  }
  const int nW = (Fb + 63) >> 6;
  for (int f0 = 0; f0 < Fb; f0 += 256) {
    const int f = f0 + tid;
    bool voiced = false;
    if (f < Fb) {
      const float pv = p[f];
      voiced = pv > 0.f;
      if (voiced) d[f] = log2f(pv) - r.mean;
    }
    const unsigned long long m = __ballot(voiced);
    if ((tid & 63) == 0 && (f >> 6) < nW) bal[f >> 6] = m;   // (a wave wholly behind F_b has no word)
  }
  __syncthreads();
  if (tid < nW) {
    int last = -1, first = -1;
    for (int j = tid - 1; j >= 0; --j) {
      const unsigned long long m = bal[j];
      if (m) {
        last = (j << 6) + 63 - __clzll((long long)m);
        break;
      }
    }
    for (int j = tid + 1; j < nW; ++j) {
      const unsigned long long m = bal[j];
      if (m) {
        first = (j << 6) + __ffsll((long long)m) - 1;
        break;
      }
    }
    before[tid] = last;
    after[tid] = first;
  }
  __syncthreads();
  for (int f = tid; f < Fb; f += 256) {
    const int w = f >> 6, bit = f & 63;
    const unsigned long long m = bal[w];
    if ((m >> bit) & 1ull) continue;
    const unsigned long long below = m & ((1ull << bit) - 1ull);
    const unsigned long long above = bit == 63 ? 0ull : (m >> (bit + 1)) << (bit + 1);
    const int pi = below ? (w << 6) + 63 - __clzll((long long)below) : before[w];
    const int ni = above ? (w << 6) + __ffsll((long long)above) - 1 : after[w];
    float v;
    if (pi >= 0 && ni >= 0) {
      const float t = __fdiv_rn((float)(f - pi), (float)(ni - pi));
      const float dp = d[pi], dn = d[ni];
      v = dp + t * (dn - dp);
    } else {
      v = d[pi >= 0 ? pi : ni];   // (count > 0: one of them exists)
    }
    d[f] = v;
  }
  __syncthreads();
  const float km1 = (float)kq * (1.0f / 65536.0f) - 1.0f;   // exact: kq has 19 bits
  const float norm = (float)((W + 1) * (W + 1));
  for (int f = tid; f < Fb; f += 256) {
    float acc = 0.f;
    for (int j = -W; j <= W; ++j) {
      int i = f + j;
      i = i < 0 ? 0 : (i > Fb - 1 ? Fb - 1 : i);
      acc = acc + (float)(W + 1 - (j < 0 ? -j : j)) * d[i];
    }
    const float s = __fdiv_rn(acc, norm);
    float e = km1 * s;
    e = fminf(fmaxf(e, -limit), limit);
    if (base) e = e + log2f((float)clamp_pitch_step(base[f]) * (1.0f / 65536.0f));
    float y = rintf(65536.0f * exp2f(e));
    y = fminf(fmaxf(y, (float)TACO_PITCH_MIN_STEP), (float)TACO_PITCH_MAX_STEP);   // (clamped as a float: a NaN becomes MIN_STEP)
    out[f] = (int)y;
  }
}

}  // namespace

extern "C" int taco_f0_range_curve(const float* period, const int32_t* frames, int frames_per_unit, const int32_t* scale_q,
                                   const int32_t* base_q, int smooth, float limit, int32_t* step_q, float* stats, int B, int F,
                                   void* stream) {
  TACO_REQUIRE(period, "f0_range_curve: period is NULL");
  TACO_REQUIRE(step_q, "f0_range_curve: step_q is NULL");
  TACO_REQUIRE(B > 0, "f0_range_curve: B=%d must be positive", B);
  TACO_REQUIRE(F > 0 && F <= TACO_STRETCH_MAX_FRAMES, "f0_range_curve: F=%d must be in 1..%d", F, TACO_STRETCH_MAX_FRAMES);
  TACO_REQUIRE(frames_per_unit >= 1, "f0_range_curve: frames_per_unit=%d must be >= 1", frames_per_unit);
  TACO_REQUIRE(smooth >= 0 && smooth <= TACO_F0_RANGE_MAX_SMOOTH, "f0_range_curve: smooth=%d must be in 0..%d", smooth,
               TACO_F0_RANGE_MAX_SMOOTH);
  TACO_REQUIRE(limit > 0.f && limit <= 1.f, "f0_range_curve: limit=%g octaves must be in (0, 1]", (double)limit);   // (NaN fails both)
  const uint64_t bytes = (uint64_t)B * (uint64_t)F * 4;
  TACO_REQUIRE(!bytes_meet(step_q, bytes, period, bytes), "f0_range_curve: step_q overlaps period");
  TACO_REQUIRE(!base_q || !bytes_meet(step_q, bytes, base_q, bytes), "f0_range_curve: step_q overlaps base_q");
  TACO_KLAUNCH(f0_range_curve_kernel, dim3((unsigned)B), dim3(256), 0, as_stream(stream), period, frames, frames_per_unit, scale_q,
               base_q, smooth, limit, step_q, stats, F);
  TACO_LAUNCH_CHECK("f0_range_curve");
  return TACO_OK;
}
