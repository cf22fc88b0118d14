// frames.h -- what the units that work on the magnitude frames of a batch (frames.hip, phase_init.hip, f0_viterbi.hip,
// f0_curve.hip) share: the length of a row, and the statistics of a pitch track's row.  Device code only, inlined into its caller.
// vocoder.hip keeps its own row_frames: there a row below 5 frames has none (the reflect padding), which is another rule.
#pragma once
#include "common.h"

// frames of row b: F without a frames array, else frames_per_unit times frames[b], clamped to [0, F]
__device__ __forceinline__ int row_frames(const int32_t* __restrict__ frames, int frames_per_unit, int b, int F) {
  if (!frames) return F;
  const int64_t n = (int64_t)frames[b] * frames_per_unit;
  return n < 0 ? 0 : (n > F ? F : (int)n);
}
// the same in a scalar register, for a caller whose branches, trip counts and barriers rest on it
__device__ __forceinline__ int row_frames_uniform(const int32_t* __restrict__ frames, int frames_per_unit, int b, int F) {
  return __builtin_amdgcn_readfirstlane(row_frames(frames, frames_per_unit, b, F));
}

// What taco_f0_stats says of one row of a pitch track, by a workgroup of 256 threads: x_f = log2(p[f]) -- or log2(o[f]) - log2(p[f])
// with o -- over the frames f < Fb with p[f] > 0 (and o[f] > 0).  Two passes (the sum, then the squares around the mean), a thread's
// frames in ascending order and the threads' partials down a fixed tree over red / cnt (256 entries each, the caller's LDS): no
// atomics.  Every thread gets the count, the mean (0 at count 0) and the sum of the squares; the deviation is sqrtf(ss / n).  f0_stats_kernel
// and f0_range_curve_kernel both call it, so the centre of the one has the bits of the other.  It ends behind a barrier; a caller
// that writes red again puts another one in front of that.
struct F0RowStats {
  int n;
  float mean, ss;
};
__device__ __forceinline__ F0RowStats f0_row_stats(const float* __restrict__ p, const float* __restrict__ o, int Fb, int tid,
                                                   float* red, int* cnt) {
  float s = 0.f;
  int c = 0;
  for (int f = tid; f < Fb; f += 256) {
    const float pv = p[f], ov = o ? o[f] : 1.0f;
    if (pv > 0.f && ov > 0.f) {
      s += o ? log2f(ov) - log2f(pv) : log2f(pv);
      ++c;
    }
  }
  red[tid] = s;
  cnt[tid] = c;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
      red[tid] += red[tid + w];
      cnt[tid] += cnt[tid + w];
    }
    __syncthreads();
  }
  const int n = cnt[0];
  const float mean = n > 0 ? red[0] / (float)n : 0.f;
  __syncthreads();
  s = 0.f;
  for (int f = tid; f < Fb; f += 256) {
    const float pv = p[f], ov = o ? o[f] : 1.0f;
    if (pv > 0.f && ov > 0.f) {
      const float x = (o ? log2f(ov) - log2f(pv) : log2f(pv)) - mean;
      s += x * x;
    }
  }
  red[tid] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  return {n, mean, red[0]};
}
