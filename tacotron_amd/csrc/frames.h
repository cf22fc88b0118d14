// frames.h -- what the units that work on the magnitude frames of a batch (frames.hip, phase_init.hip, f0_viterbi.hip) share: the
// length of a row.  Device code only, inlined into its caller.  vocoder.hip keeps its own row_frames: there a row below 5 frames
// has none (the reflect padding), which is another rule.
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
