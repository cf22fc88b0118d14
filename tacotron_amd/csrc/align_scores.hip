// align_scores.hip -- read-outs over stored alignments (B, Td, Tt): the end-detection rule of taco_infer_stop for decodes that ran
// to Td (launch_stop_rule, called by model.hip) and the per-utterance attention scores (include/taco_hip.h taco_alignment_scores).
// One workgroup per batch row in both; the argmax of a step is taken under one total order (value desc, index asc).
#include "common.h"
#include "kernels.h"

namespace {

// The end-detection rule of include/taco_hip.h (TacoStopRule) over stored alignments: one workgroup per batch row walks t in
// order.  a_t = first index of max_s alignments[b, t, s] over s < Tt (lowest index on ties: lane-local ascending scan, then a
// wave butterfly and a fixed-order pass over the four waves, all under the one total order (value desc, index asc)).
__global__ __launch_bounds__(256) void stop_rule_kernel(const float* __restrict__ align, const int32_t* __restrict__ text_length,
                                                        int32_t* __restrict__ len_out, int Tt, int Td, int end_offset, int hold,
                                                        int min_steps) {
  __shared__ float wv[4];
  __shared__ int wi[4];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int L = text_length[b];
  L = L < 1 ? 1 : (L > Tt ? Tt : L);
  const int target = L - 1 - end_offset > 0 ? L - 1 - end_offset : 0;
  int run = 0, len = Td;
  for (int t = 0; t < Td; ++t) {
    const float* al = align + ((int64_t)b * Td + t) * Tt;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int s = threadIdx.x; s < Tt; s += 256) {
      const float v = al[s];
      if (v > bv) bv = v, bi = s;
    }
    for (int o = 32; o; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
    }
    if (lane == 0) wv[wave] = bv, wi[wave] = bi;
    __syncthreads();
    bv = wv[0], bi = wi[0];
    for (int w = 1; w < 4; ++w)
      if (wv[w] > bv || (wv[w] == bv && wi[w] < bi)) bv = wv[w], bi = wi[w];
    __syncthreads();   // (wv / wi are rewritten in the next step)
    run = bi >= target ? run + 1 : 0;
    if (run >= hold && t + 1 >= min_steps) {   // (uniform: every thread holds the same run)
      len = min(Td, (t + 4) / 4 * 4);
      break;
    }
  }
  if (threadIdx.x == 0) len_out[b] = len;
}

// ---- alignment scores (include/taco_hip.h taco_alignment_scores) ------------------------------------------------------------------
// One workgroup of 16 waves per batch row, one launch, no workspace: the row's a_t record has to meet in one place for `back`,
// `skip` and `covered`, and 2 bytes per step fit the LDS of one workgroup, so nothing is handed from one workgroup to another.
// Unlike the stop rule there is no run counter: a step's (a_t, p_t, pad sum) depends on that step alone, so wave w takes the steps
// w, w + 16, ... on its own -- 64 lanes over Tt, 16-byte loads when Tt % 4 == 0 and the base is 16-byte aligned (every step then
// starts on a 16-byte boundary), 4-byte loads otherwise -- and the load of its next step is in flight while it reduces this one.
// The argmax is reduced on the DPP path under the total order (value desc, index asc): associative, commutative and idempotent, so
// the rotations of wave_max apply unchanged.  NaN elements never win a comparison; an all-NaN step keeps the sentinel index.
// Phase 2 walks the record 64 steps per wave with ballots and popcounts; `covered` is the popcount of an LDS bitmap that phase 1
// fills with ds_or (idempotent: no order dependence).  The two means are summed per wave in step order and over the waves in wave
// order: the same arguments give the same bits.
constexpr int kAlignWaves = 16;
constexpr int kAlignThreads = 64 * kAlignWaves;
constexpr int kAlignNone = 0x7fffffff;   // index of "no non-NaN element yet": loses every tie

template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ void argmax_dpp(float& bv, int& bi) {
  const float ov = dpp_move<CTRL, ROW_MASK>(bv, bv);   // (lanes outside the row mask and lanes without a source keep their own pair)
  const int oi = __builtin_amdgcn_update_dpp(bi, bi, CTRL, ROW_MASK, 0xf, false);
  if (ov > bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
}
__device__ __forceinline__ void wave_argmax(float& bv, int& bi) {
  argmax_dpp<0xb1>(bv, bi);          // quad_perm [1,0,3,2]
  argmax_dpp<0x4e>(bv, bi);          // quad_perm [2,3,0,1]
  argmax_dpp<0x124>(bv, bi);         // row_ror:4
  argmax_dpp<0x128>(bv, bi);         // row_ror:8
  argmax_dpp<0x142, 0xa>(bv, bi);    // row_bcast:15 -> rows 1,3
  argmax_dpp<0x143, 0xc>(bv, bi);    // row_bcast:31 -> rows 2,3
  bv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(bv), 63));
  bi = __builtin_amdgcn_readlane(bi, 63);
}
__device__ __forceinline__ void align_take(float v, int s, int L, float& bv, int& bi, float& pad) {
  if (v > bv || (v == bv && s < bi)) bv = v, bi = s;   // (both false for a NaN)
  if (s >= L) pad += v;
}
// item i of a step: VEC: elements 4 i .. 4 i + 3 in one 16-byte load; else element i
template <bool VEC>
__device__ __forceinline__ f32x4 align_load(const float* __restrict__ al, int i) {
  if (VEC) return *reinterpret_cast<const f32x4*>(al + 4 * i);
  f32x4 v = {al[i], 0.f, 0.f, 0.f};
  return v;
}
template <bool VEC>
__device__ __forceinline__ void align_scan(f32x4 v, int i, int L, float& bv, int& bi, float& pad) {
  if (VEC) {
    align_take(v.x, 4 * i, L, bv, bi, pad);
    align_take(v.y, 4 * i + 1, L, bv, bi, pad);
    align_take(v.z, 4 * i + 2, L, bv, bi, pad);
    align_take(v.w, 4 * i + 3, L, bv, bi, pad);
  } else {
    align_take(v.x, i, L, bv, bi, pad);
  }
}
__device__ __forceinline__ int wave_imax(int v) {
  for (int o = 32; o; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_isum(int v) {
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <bool VEC>
__global__ __launch_bounds__(kAlignThreads) void alignment_scores_kernel(const float* __restrict__ align,
                                                                         const int32_t* __restrict__ text_length,
                                                                         const int32_t* __restrict__ steps, int max_jump,
                                                                         int32_t* __restrict__ counts, float* __restrict__ means, int Td,
                                                                         int Tt) {
  __shared__ uint16_t rec[TACO_ALIGNMENT_MAX_TD];          // a_t of the scored steps
  __shared__ uint32_t seen[TACO_ALIGNMENT_MAX_TT / 32];    // bit s: a_t == s for some scored t (s < L only)
  __shared__ float wsum[kAlignWaves][2];
  __shared__ int wcnt[kAlignWaves][5];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int L = text_length[b];
  L = L < 1 ? 1 : (L > Tt ? Tt : L);
  int n = steps ? steps[b] : Td;
  n = n < 0 ? 0 : (n > Td ? Td : n);
  const int words = (L + 31) >> 5;
  for (int w = threadIdx.x; w < words; w += kAlignThreads) seen[w] = 0u;
  __syncthreads();

  // phase 1: a wave per step
  const float* row = align + (int64_t)b * Td * Tt;
  const int items = VEC ? Tt >> 2 : Tt;
  float fsum = 0.f, psum = 0.f;
  f32x4 cur = {0.f, 0.f, 0.f, 0.f};
  if (wave < n && lane < items) cur = align_load<VEC>(row + (int64_t)wave * Tt, lane);
  for (int t = wave; t < n; t += kAlignWaves) {   // (wave-uniform trip count: every lane reaches the DPP reductions)
    const float* al = row + (int64_t)t * Tt;
    f32x4 nxt = {0.f, 0.f, 0.f, 0.f};
    if (t + kAlignWaves < n && lane < items) nxt = align_load<VEC>(al + (int64_t)kAlignWaves * Tt, lane);
    float bv = -INFINITY, pad = 0.f;
    int bi = kAlignNone;
    if (lane < items) align_scan<VEC>(cur, lane, L, bv, bi, pad);
    for (int i = lane + 64; i < items; i += 64) align_scan<VEC>(align_load<VEC>(al, i), i, L, bv, bi, pad);
    wave_argmax(bv, bi);
    pad = wave_sum(pad);
    const bool none = bi == kAlignNone;                    // every element is NaN: a_t = 0 and p_t = a[t, 0], a NaN
    const int a = none ? 0 : bi;
    fsum += none ? __builtin_nanf("") : bv;
    psum += pad;
    if (lane == 0) {
      rec[t] = (uint16_t)a;
      if (a < L) atomicOr(&seen[a >> 5], 1u << (a & 31));
    }
    cur = nxt;
  }
  if (lane == 0) wsum[wave][0] = fsum, wsum[wave][1] = psum;
  __syncthreads();

  // phase 2: the record, 64 steps per wave and pass
  int end = 0, n_pad = 0, n_back = 0, n_skip = 0;
  for (int t0 = wave * 64; t0 < n; t0 += kAlignThreads) {
    const int t = t0 + lane;
    const bool in = t < n;
    const int a = in ? (int)rec[t] : 0;
    const int prev = in && t > 0 ? (int)rec[t - 1] : a;
    end = max(end, a);
    n_pad += __popcll(__ballot(in && a >= L));
    n_back += __popcll(__ballot(in && a < prev));
    n_skip += __popcll(__ballot(in && a - prev > max_jump));
  }
  end = wave_imax(end);
  int cov = 0;
  for (int w = threadIdx.x; w < words; w += kAlignThreads) cov += __popc(seen[w]);
  cov = wave_isum(cov);
  if (lane == 0) wcnt[wave][0] = end, wcnt[wave][1] = n_pad, wcnt[wave][2] = n_back, wcnt[wave][3] = n_skip, wcnt[wave][4] = cov;
  __syncthreads();
  if (threadIdx.x == 0) {
    int c[5] = {0, 0, 0, 0, 0};
    float f = 0.f, p = 0.f;
    for (int w = 0; w < kAlignWaves; ++w) {
      c[0] = max(c[0], wcnt[w][0]);
      for (int k = 1; k < 5; ++k) c[k] += wcnt[w][k];
      f += wsum[w][0];
      p += wsum[w][1];
    }
    int32_t* co = counts + (int64_t)b * 6;
    co[0] = n;
    for (int k = 0; k < 5; ++k) co[1 + k] = c[k];
    means[(int64_t)b * 2] = n ? f / (float)n : 0.f;
    means[(int64_t)b * 2 + 1] = n ? p / (float)n : 0.f;
  }
}

}  // namespace

int launch_stop_rule(const float* align, const int32_t* text_length, int32_t* len, int B, int Tt, int Td, int end_offset, int hold,
                     int min_steps, hipStream_t s) {
  TACO_KLAUNCH(stop_rule_kernel, dim3(B), dim3(256), 0, s, align, text_length, len, Tt, Td, end_offset, hold, min_steps);
  TACO_LAUNCH_CHECK("stop_rule");
  return TACO_OK;
}
static int launch_alignment_scores(const float* align, const int32_t* text_length, const int32_t* steps, int max_jump, int32_t* counts,
                            float* means, int B, int Td, int Tt, hipStream_t s) {
  if (Tt % 4 == 0 && (reinterpret_cast<uintptr_t>(align) & 15) == 0)
    TACO_KLAUNCH(alignment_scores_kernel<true>, dim3(B), dim3(kAlignThreads), 0, s, align, text_length, steps, max_jump, counts, means,
                 Td, Tt);
  else
    TACO_KLAUNCH(alignment_scores_kernel<false>, dim3(B), dim3(kAlignThreads), 0, s, align, text_length, steps, max_jump, counts, means,
                 Td, Tt);
  TACO_LAUNCH_CHECK("alignment_scores");
  return TACO_OK;
}
extern "C" int taco_alignment_scores(const float* alignments, const int32_t* text_length, const int32_t* steps, int max_jump,
                                     int32_t* counts, float* means, int B, int Td, int Tt, void* stream) {
  TACO_REQUIRE(alignments, "alignment_scores: alignments is NULL");
  TACO_REQUIRE(text_length, "alignment_scores: text_length is NULL");
  TACO_REQUIRE(counts, "alignment_scores: counts is NULL");
  TACO_REQUIRE(means, "alignment_scores: means is NULL");
  TACO_REQUIRE(B > 0, "alignment_scores: B=%d must be positive", B);
  TACO_REQUIRE(Td > 0, "alignment_scores: Td=%d must be positive", Td);
  TACO_REQUIRE(Tt > 0, "alignment_scores: Tt=%d must be positive", Tt);
  TACO_REQUIRE(max_jump >= 0, "alignment_scores: max_jump=%d is negative", max_jump);
  TACO_REQUIRE(Td <= TACO_ALIGNMENT_MAX_TD, "alignment_scores: Td=%d is above the %d steps one record holds", Td, TACO_ALIGNMENT_MAX_TD);
  TACO_REQUIRE(Tt <= TACO_ALIGNMENT_MAX_TT, "alignment_scores: Tt=%d is above the %d characters one bitmap holds", Tt, TACO_ALIGNMENT_MAX_TT);
  return launch_alignment_scores(alignments, text_length, steps, max_jump, counts, means, B, Td, Tt, as_stream(stream));
}
