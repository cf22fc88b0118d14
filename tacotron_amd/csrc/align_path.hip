// align_path.hip -- the best monotone path through an attention matrix (include/taco_hip.h taco_alignment_path): per batch row the
// path of largest attention mass that starts on character 0, never goes back and advances by at most max_jump characters per
// decoder step, its per-character durations, its end and its mass.  No counterpart in the reference, which only draws the matrix.
//
// The work is a latency chain: Td dependent steps per row, a few hundred cells each, 32 independent rows.  One workgroup per row,
// one launch; what a step costs is what the call costs, so both forms below go after the step and not after bandwidth.
//
// Wave form (Tt <= 256 and the direction table fits LDS -- every shape the product decodes): ONE wave owns the row, four
// consecutive characters per lane, the previous row of Q in registers.  The up-to-J lower neighbours of a lane's four cells sit in
// the ceil(J / 4) lanes below it and come over by DPP wave_shr:1 (a VALU move; lane 0 keeps the "unreachable" sentinel), so a step
// has no LDS round trip and no barrier.  The alignment rows of the next eight steps are in flight while a step is computed (16 bytes
// per lane where Tt % 4 == 0 and the base allows, four 4-byte loads otherwise): a step is a fraction of one load's latency.  The
// four direction bytes of a lane go to LDS as one dword.
//
// General form (any Tt up to the limit, any Td): the two live rows of Q in LDS with 16 sentinel cells in front, so that the
// predecessor loop has no bounds branch; one lds_barrier() per step (two buffers are enough: step t writes the buffer step t - 1
// read, and every wave has passed the barrier between them); a direction byte per cell to the row's slice of the workspace, stores
// nobody waits for until the backtrack.
//
// Unreachable cells hold -1: every reachable Q is a sum of non-negative weights, so a sentinel never wins a comparison against a
// reachable candidate, and every reachable cell has one (header, "Reachability").  The predecessor scan runs d = 0, 1, .. and
// replaces on strictly larger only: the smallest d wins ties.
//
// Both forms end alike: argmax of the last row (value descending, index ascending), one lane walks the direction table backwards
// into an LDS copy of the path, and the workgroup writes path, and dur from the run boundaries of the path: the lane at a run's
// first step subtracts t from the character's counter, the lane at its last step adds t + 1 (integer LDS atomics: no order
// dependence).  skipped = end + 1 - number of runs.
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr size_t kPathLdsBudget = 128 * 1024;
constexpr int kPathWaveTt = 256;   // widest row one wave holds, four characters per lane
constexpr int kPathFront = 16;     // sentinel cells in front of a Q row of the general form (> TACO_ALIGN_PATH_MAX_JUMP)
constexpr int kPathMaxThreads = 1024;
constexpr int kPathAhead = 8;     // alignment rows in flight per lane of the single-wave form

struct PathPlan {
  bool wave;          // the single-wave form
  size_t lds_bytes;   // dynamic LDS of the launch
  int threads;
  int64_t row_bytes;  // workspace bytes per row (0: none)
};
// dynamic LDS, both forms: [form's own part] | dur counters int32 [Tt] | path uint16 [Td rounded up to 2]
inline size_t path_tail_bytes(int Td, int Tt) { return (size_t)Tt * 4 + (size_t)((Td + 1) & ~1) * 2; }
PathPlan path_plan(int Td, int Tt) {
  PathPlan p;
  const size_t table = (size_t)Td * ((Tt + 3) >> 2) * 4;
  p.wave = Tt <= kPathWaveTt && table + path_tail_bytes(Td, Tt) <= kPathLdsBudget;
  if (p.wave) {
    p.lds_bytes = table + path_tail_bytes(Td, Tt);
    p.threads = 64;
    p.row_bytes = 0;
  } else {
    p.lds_bytes = (size_t)2 * (kPathFront + Tt) * 4 + path_tail_bytes(Td, Tt);
    p.threads = (Tt + 63) / 64 * 64;
    if (p.threads > kPathMaxThreads) p.threads = kPathMaxThreads;
    p.row_bytes = (int64_t)Td * Tt;
  }
  return p;
}
// workspace of taco_alignment_path: a direction byte per cell of each row's (Td, Tt) table (none in the single-wave form)
struct PathWs {
  uint8_t* way;
  int64_t bytes;
};
PathWs path_ws(void* ws, int B, int Td, int Tt) {
  WsCarver c(ws);
  PathWs w;
  w.way = c.take<uint8_t>(B * path_plan(Td, Tt).row_bytes);
  w.bytes = c.bytes;
  return w;
}
bool path_shape_ok(int B, int Td, int Tt) {
  return B > 0 && Td > 0 && Tt > 0 && Td <= TACO_ALIGN_PATH_MAX_TD && Tt <= TACO_ALIGN_PATH_MAX_TT;
}

__device__ __forceinline__ float path_weight(float a) { return a > 0.f ? a : 0.f; }   // (NaN, negatives and -0 give +0)

__device__ __forceinline__ void path_row_args(const int32_t* __restrict__ text_length, const int32_t* __restrict__ steps, int b, int Td,
                                              int Tt, int& L, int& n) {
  L = text_length[b];
  L = L < 1 ? 1 : (L > Tt ? Tt : L);
  n = steps ? steps[b] : Td;
  n = n < 0 ? 0 : (n > Td ? Td : n);
  L = __builtin_amdgcn_readfirstlane(L);   // the same for every lane: trip counts and barriers are uniform
  n = __builtin_amdgcn_readfirstlane(n);
}

__device__ __forceinline__ void path_argmax_take(float ov, int oi, float& bv, int& bi) {
  if (ov > bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
}
__device__ __forceinline__ void path_wave_argmax(float& bv, int& bi) {   // once per row: the shuffle path will do
  for (int o = 32; o; o >>= 1) path_argmax_take(__shfl_xor(bv, o, 64), __shfl_xor(bi, o, 64), bv, bi);
}

__device__ __forceinline__ void path_empty_row(int32_t* __restrict__ path, int32_t* __restrict__ dur, int32_t* __restrict__ counts,
                                               float* __restrict__ mass, int Td, int Tt) {
  for (int t = threadIdx.x; t < Td; t += blockDim.x) path[t] = -1;
  for (int s = threadIdx.x; s < Tt; s += blockDim.x) dur[s] = 0;
  if (threadIdx.x == 0) counts[0] = 0, counts[1] = 0, counts[2] = 0, mass[0] = 0.f;
}

// Behind the backtrack: pl[0 .. n) holds the path, dur_l[0 .. Tt) is zero, every thread of the workgroup is here.
__device__ __forceinline__ void path_finish(const uint16_t* pl, int* dur_l, int* runs_l, int n, int e, float q, int32_t* __restrict__ path,
                                            int32_t* __restrict__ dur, int32_t* __restrict__ counts, float* __restrict__ mass, int Td,
                                            int Tt) {
  int runs = 0;
  for (int t = threadIdx.x; t < Td; t += blockDim.x) {
    int p = -1;
    if (t < n) {
      p = pl[t];
      p = p < Tt ? p : Tt - 1;   // (it is below L; the bounds of the LDS counters do not rest on the table's contents)
      const bool first = t == 0 || pl[t - 1] != pl[t], last = t == n - 1 || pl[t + 1] != pl[t];
      if (first) atomicSub(&dur_l[p], t), ++runs;
      if (last) atomicAdd(&dur_l[p], t + 1);
    }
    path[t] = p;
  }
  if (runs) atomicAdd(runs_l, runs);
  __syncthreads();
  for (int s = threadIdx.x; s < Tt; s += blockDim.x) dur[s] = dur_l[s];
  if (threadIdx.x == 0) counts[0] = n, counts[1] = e, counts[2] = e + 1 - *runs_l, mass[0] = q;
}

// ---- the wave form ----------------------------------------------------------------------------------------------------------------
// The four cells of a lane, loaded without a branch so that the loads of several steps stay in flight with counted waits: a lane
// whose cells lie behind the row reads the row's last cells instead (what a cell >= L holds never reaches a result).
template <bool VEC>
__device__ __forceinline__ f32x4 path_load4(const float* __restrict__ al, int s0, int Tt) {
  if (VEC) return *reinterpret_cast<const f32x4*>(al + min(s0, Tt - 4));   // (Tt % 4 == 0 and Tt >= 4)
  const int last = Tt - 1;
  f32x4 v = {al[min(s0, last)], al[min(s0 + 1, last)], al[min(s0 + 2, last)], al[min(s0 + 3, last)]};
  return v;
}

// One step of the single-wave form: q holds Q(t-1, .) of the lane's four cells and leaves as Q(t, .); -> the four direction bytes.
// FULL: J == 4 NL (the default J = 4 among them), every candidate the NL lanes hold is admissible and the test against J goes
template <int NL, bool FULL>
__device__ __forceinline__ uint32_t path_wave_step(float (&q)[4], f32x4 cur, int t, int s0, int L, int J) {
  // c[4 NL + i] = Q(t-1, s0 + i); c[4 NL + i - d] = Q(t-1, s0 + i - d), the sentinel in front of character 0
  float c[4 * NL + 4];
  float sh[4] = {q[0], q[1], q[2], q[3]};
#pragma unroll
  for (int i = 0; i < 4; ++i) c[4 * NL + i] = q[i];
#pragma unroll
  for (int j = 1; j <= NL; ++j) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      sh[i] = dpp_move<0x138>(-1.f, sh[i]);   // wave_shr:1 -- lane l <- lane l - 1, lane 0 keeps -1
      c[4 * (NL - j) + i] = sh[i];
    }
  }
  const int lim = min(L - 1, J * t);
  const float a[4] = {cur.x, cur.y, cur.z, cur.w};
  uint32_t word = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float best = c[4 * NL + i];
    uint32_t bd = 0;
#pragma unroll
    for (int d = 1; d <= 4 * NL; ++d) {
      const float x = c[4 * NL + i - d];
      if ((FULL || d <= J) && x > best) best = x, bd = d;
    }
    q[i] = s0 + i <= lim ? path_weight(a[i]) + best : -1.f;
    word |= bd << (8 * i);
  }
  return word;
}

// NL = ceil(J / 4): how many lanes below hold candidates; FULL: J == 4 NL
template <bool VEC, int NL, bool FULL>
__global__ __launch_bounds__(64) void alignment_path_wave_kernel(const float* __restrict__ align, const int32_t* __restrict__ text_length,
                                                                 const int32_t* __restrict__ steps, int J, int32_t* __restrict__ path,
                                                                 int32_t* __restrict__ dur, int32_t* __restrict__ counts,
                                                                 float* __restrict__ mass, int Td, int Tt) {
  extern __shared__ __attribute__((aligned(16))) uint32_t ap_lds[];   // dirs [Td][W] dwords | dur_l [Tt] | pl [Td]
  __shared__ int runs_l;
  const int b = blockIdx.x, lane = threadIdx.x, W = (Tt + 3) >> 2, s0 = 4 * lane;
  int L, n;
  path_row_args(text_length, steps, b, Td, Tt, L, n);
  path += (int64_t)b * Td, dur += (int64_t)b * Tt, counts += (int64_t)b * 3, mass += b;
  if (n == 0) {
    path_empty_row(path, dur, counts, mass, Td, Tt);
    return;
  }
  uint32_t* dirs = ap_lds;
  int* dur_l = reinterpret_cast<int*>(ap_lds + (size_t)Td * W);
  uint16_t* pl = reinterpret_cast<uint16_t*>(dur_l + Tt);
  for (int s = lane; s < Tt; s += 64) dur_l[s] = 0;
  if (lane == 0) runs_l = 0;

  const float* row = align + (int64_t)b * Td * Tt;
  float q[4] = {-1.f, -1.f, -1.f, -1.f};
  if (lane == 0) q[0] = path_weight(row[0]);
  // the alignment rows of the next kPathAhead steps are in flight: a step computes in a fraction of a load's latency.  Rows past
  // n - 1 are read as row n - 1 (inside the tensor, never used), so the main loop has no branch around a load
  f32x4 ahead[kPathAhead];
#pragma unroll
  for (int k = 0; k < kPathAhead; ++k) ahead[k] = path_load4<VEC>(row + (int64_t)min(1 + k, n - 1) * Tt, s0, Tt);
  int t0 = 1;
  for (; t0 + kPathAhead <= n; t0 += kPathAhead) {
#pragma unroll
    for (int k = 0; k < kPathAhead; ++k) {
      const int t = t0 + k;
      const f32x4 cur = ahead[k];
      ahead[k] = path_load4<VEC>(row + (int64_t)min(t + kPathAhead, n - 1) * Tt, s0, Tt);
      const uint32_t word = path_wave_step<NL, FULL>(q, cur, t, s0, L, J);
      if (lane < W) dirs[t * W + lane] = word;
    }
  }
#pragma unroll
  for (int k = 0; k < kPathAhead - 1; ++k) {   // the last n - t0 < kPathAhead steps: their rows are loaded
    const int t = t0 + k;
    if (t >= n) break;   // (uniform)
    const uint32_t word = path_wave_step<NL, FULL>(q, ahead[k], t, s0, L, J);
    if (lane < W) dirs[t * W + lane] = word;
  }

  // the free end: lowest s of the largest Q(n-1, s); reachable cells are >= 0, the rest -1, and cell 0 is always reachable
  float bv = q[0];
  int bi = s0;
#pragma unroll
  for (int i = 1; i < 4; ++i) path_argmax_take(q[i], s0 + i, bv, bi);
  path_wave_argmax(bv, bi);
  const int e = min(max(bi, 0), L - 1);
  __syncthreads();   // (one wave: the direction dwords are in LDS before lane 0 reads them)
  if (lane == 0) {
    int s = e;
    for (int t = n - 1; t >= 1; --t) {
      pl[t] = (uint16_t)s;
      const int d = (dirs[t * W + (s >> 2)] >> (8 * (s & 3))) & 0xff;
      s = s - d > 0 ? s - d : 0;
    }
    pl[0] = (uint16_t)s;
  }
  __syncthreads();
  path_finish(pl, dur_l, &runs_l, n, e, bv, path, dur, counts, mass, Td, Tt);
}

// ---- the general form -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPathMaxThreads) void alignment_path_block_kernel(const float* __restrict__ align,
                                                                               const int32_t* __restrict__ text_length,
                                                                               const int32_t* __restrict__ steps, int J,
                                                                               int32_t* __restrict__ path, int32_t* __restrict__ dur,
                                                                               int32_t* __restrict__ counts, float* __restrict__ mass,
                                                                               uint8_t* ws, int Td, int Tt) {
  extern __shared__ __attribute__((aligned(16))) uint32_t ap_lds[];   // Q [2][kPathFront + Tt] | dur_l [Tt] | pl [Td]
  __shared__ int runs_l;
  __shared__ float wv[kPathMaxThreads / 64];
  __shared__ int wi[kPathMaxThreads / 64];
  const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x, stride = kPathFront + Tt;
  int L, n;
  path_row_args(text_length, steps, b, Td, Tt, L, n);
  path += (int64_t)b * Td, dur += (int64_t)b * Tt, counts += (int64_t)b * 3, mass += b;
  if (n == 0) {
    path_empty_row(path, dur, counts, mass, Td, Tt);
    return;
  }
  float* Q = reinterpret_cast<float*>(ap_lds);
  int* dur_l = reinterpret_cast<int*>(ap_lds + 2 * stride);
  uint16_t* pl = reinterpret_cast<uint16_t*>(dur_l + Tt);
  uint8_t* dirs = ws + (int64_t)b * Td * Tt;
  const float* row = align + (int64_t)b * Td * Tt;
  for (int i = tid; i < 2 * stride; i += nthr) Q[i] = -1.f;
  for (int s = tid; s < Tt; s += nthr) dur_l[s] = 0;
  if (tid == 0) runs_l = 0;
  __syncthreads();
  if (tid == 0) Q[kPathFront] = path_weight(row[0]);
  float cur = 0.f;
  if (n > 1 && tid <= min(L - 1, J)) cur = row[Tt + tid];
  for (int t = 1; t < n; ++t) {
    lds_barrier();   // step t - 1 is written, and nobody still reads the buffer this step writes
    const float* prev = Q + ((t - 1) & 1) * stride + kPathFront;
    float* now = Q + (t & 1) * stride + kPathFront;
    const int lim = min(L - 1, J * t);
    float nxt = 0.f;
    if (t + 1 < n && tid <= min(L - 1, J * (t + 1))) nxt = row[(int64_t)(t + 1) * Tt + tid];
    const float* al = row + (int64_t)t * Tt;
    uint8_t* dr = dirs + (int64_t)t * Tt;
    for (int s = tid; s <= lim; s += nthr) {
      const float a = s == tid ? cur : al[s];
      float best = prev[s];
      int bd = 0;
      for (int d = 1; d <= J; ++d) {   // (s - d >= -kPathFront: the sentinels in front)
        const float x = prev[s - d];
        if (x > best) best = x, bd = d;
      }
      now[s] = path_weight(a) + best;
      dr[s] = (uint8_t)bd;
    }
    cur = nxt;
  }
  __syncthreads();
  const float* fin = Q + ((n - 1) & 1) * stride + kPathFront;
  float bv = -1.f;
  int bi = 0x7fffffff;
  for (int s = tid; s < L; s += nthr) path_argmax_take(fin[s], s, bv, bi);
  path_wave_argmax(bv, bi);
  if ((tid & 63) == 0) wv[tid >> 6] = bv, wi[tid >> 6] = bi;
  // every wave's direction stores are acknowledged before one lane reads the table past the vector cache (as frame_dtw_path)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int w = 0; w < (nthr >> 6); ++w) path_argmax_take(wv[w], wi[w], bv, bi);   // (idempotent: every thread ends with the same pair)
  const int e = min(max(bi, 0), L - 1);
  if (tid == 0) {
    int s = e;
    for (int t = n - 1; t >= 1; --t) {
      pl[t] = (uint16_t)s;
      const int d = __hip_atomic_load(dirs + (int64_t)t * Tt + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s = s - d > 0 ? s - d : 0;
    }
    pl[0] = (uint16_t)s;
  }
  __syncthreads();
  path_finish(pl, dur_l, &runs_l, n, e, bv, path, dur, counts, mass, Td, Tt);
}

template <bool VEC, int NL, bool FULL>
bool launch_path_wave(size_t lds, hipStream_t s, const float* align, const int32_t* text_length, const int32_t* steps, int J, int32_t* path,
                      int32_t* dur, int32_t* counts, float* mass, int B, int Td, int Tt) {
  static DynSmemOnce raised;
  const auto kernel = alignment_path_wave_kernel<VEC, NL, FULL>;
  if (!ensure_dyn_smem(raised, reinterpret_cast<const void*>(kernel), kPathLdsBudget)) return false;
  TACO_KLAUNCH(kernel, dim3(B), dim3(64), lds, s, align, text_length, steps, J, path, dur, counts, mass, Td, Tt);
  return true;
}
template <bool VEC, bool FULL>
bool launch_path_wave(int NL, size_t lds, hipStream_t s, const float* align, const int32_t* text_length, const int32_t* steps, int J,
                      int32_t* path, int32_t* dur, int32_t* counts, float* mass, int B, int Td, int Tt) {
  switch (NL) {
    case 1: return launch_path_wave<VEC, 1, FULL>(lds, s, align, text_length, steps, J, path, dur, counts, mass, B, Td, Tt);
    case 2: return launch_path_wave<VEC, 2, FULL>(lds, s, align, text_length, steps, J, path, dur, counts, mass, B, Td, Tt);
    case 3: return launch_path_wave<VEC, 3, FULL>(lds, s, align, text_length, steps, J, path, dur, counts, mass, B, Td, Tt);
    default: return launch_path_wave<VEC, 4, FULL>(lds, s, align, text_length, steps, J, path, dur, counts, mass, B, Td, Tt);
  }
}

// ---- taco_path_curve --------------------------------------------------------------------------------------------------------------
// Per-character values along the path: curve[b, t r + u] = values[b, path[b, t]], `fill` where the path names no character of the
// row (-1 behind the row's steps, or an index >= Tt).  A pure gather, one element per thread, the r frames of a step next to each
// other: stores are contiguous, the loads of r neighbouring lanes hit one address.
__global__ __launch_bounds__(256) void path_curve_kernel(const int32_t* __restrict__ path, const int32_t* __restrict__ values, int r,
                                                          int32_t fill, int32_t* __restrict__ curve, int64_t total, int Td, int Tt) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;   // = (b Td + t) r + u
  if (e >= total) return;
  const int64_t step = e / r;
  const int64_t b = step / Td;
  const int s = path[step];
  curve[e] = (s >= 0 && s < Tt) ? values[b * Tt + s] : fill;
}

}  // namespace

extern "C" int taco_path_curve(const int32_t* path, const int32_t* values, int frames_per_step, int32_t fill, int32_t* curve, int B, int Td,
                               int Tt, void* stream) {
  TACO_REQUIRE(path, "path_curve: path is NULL");
  TACO_REQUIRE(values, "path_curve: values is NULL");
  TACO_REQUIRE(curve, "path_curve: curve is NULL");
  TACO_REQUIRE(B > 0, "path_curve: B=%d must be positive", B);
  TACO_REQUIRE(Td > 0, "path_curve: Td=%d must be positive", Td);
  TACO_REQUIRE(Tt > 0, "path_curve: Tt=%d must be positive", Tt);
  TACO_REQUIRE(frames_per_step >= 1, "path_curve: frames_per_step=%d must be >= 1", frames_per_step);
  TACO_REQUIRE((int64_t)Td * frames_per_step <= TACO_STRETCH_MAX_FRAMES, "path_curve: Td=%d x frames_per_step=%d is above the %d frames of a curve",
               Td, frames_per_step, TACO_STRETCH_MAX_FRAMES);
  const int64_t total = (int64_t)B * Td * frames_per_step;   // (< 2^31 * 2^13)
  const int64_t blocks = (total + 255) / 256;
  TACO_REQUIRE(blocks <= 0x7fffffff, "path_curve: B=%d x Td=%d x frames_per_step=%d needs more than 2^31 workgroups", B, Td, frames_per_step);
  hipStream_t s = as_stream(stream);
  TACO_KLAUNCH(path_curve_kernel, dim3((unsigned)blocks), dim3(256), 0, s, path, values, frames_per_step, fill, curve, total, Td, Tt);
  TACO_LAUNCH_CHECK("path_curve");
  return TACO_OK;
}

extern "C" int64_t taco_alignment_path_workspace_bytes(int B, int Td, int Tt) {
  if (!path_shape_ok(B, Td, Tt)) return TACO_EINVAL;
  return path_ws(nullptr, B, Td, Tt).bytes;
}

extern "C" int taco_alignment_path(const float* alignments, const int32_t* text_length, const int32_t* steps, int max_jump,
                                   int32_t* path, int32_t* dur, int32_t* counts, float* mass, void* workspace, int B, int Td, int Tt,
                                   void* stream) {
  TACO_REQUIRE(alignments, "alignment_path: alignments is NULL");
  TACO_REQUIRE(text_length, "alignment_path: text_length is NULL");
  TACO_REQUIRE(path, "alignment_path: path is NULL");
  TACO_REQUIRE(dur, "alignment_path: dur is NULL");
  TACO_REQUIRE(counts, "alignment_path: counts is NULL");
  TACO_REQUIRE(mass, "alignment_path: mass is NULL");
  TACO_REQUIRE(B > 0, "alignment_path: B=%d must be positive", B);
  TACO_REQUIRE(Td > 0, "alignment_path: Td=%d must be positive", Td);
  TACO_REQUIRE(Tt > 0, "alignment_path: Tt=%d must be positive", Tt);
  TACO_REQUIRE(Td <= TACO_ALIGN_PATH_MAX_TD, "alignment_path: Td=%d is above the %d steps one LDS path holds", Td, TACO_ALIGN_PATH_MAX_TD);
  TACO_REQUIRE(Tt <= TACO_ALIGN_PATH_MAX_TT, "alignment_path: Tt=%d is above the %d characters one LDS row holds", Tt,
               TACO_ALIGN_PATH_MAX_TT);
  TACO_REQUIRE(max_jump >= 1 && max_jump <= TACO_ALIGN_PATH_MAX_JUMP, "alignment_path: max_jump=%d is outside 1 .. %d", max_jump,
               TACO_ALIGN_PATH_MAX_JUMP);
  const PathPlan p = path_plan(Td, Tt);
  TACO_REQUIRE(p.row_bytes == 0 || workspace, "alignment_path: workspace is NULL (the direction table of this shape needs %lld bytes)",
               (long long)path_ws(nullptr, B, Td, Tt).bytes);
  hipStream_t s = as_stream(stream);
  if (p.wave) {
    const bool vec = Tt % 4 == 0 && (reinterpret_cast<uintptr_t>(alignments) & 15) == 0;
    const int NL = (max_jump + 3) / 4;
    const bool full = max_jump == 4 * NL;
#define TACO_PATH_WAVE(V, F) \
  launch_path_wave<V, F>(NL, p.lds_bytes, s, alignments, text_length, steps, max_jump, path, dur, counts, mass, B, Td, Tt)
    const bool ok = vec ? (full ? TACO_PATH_WAVE(true, true) : TACO_PATH_WAVE(true, false))
                        : (full ? TACO_PATH_WAVE(false, true) : TACO_PATH_WAVE(false, false));
#undef TACO_PATH_WAVE
    if (!ok) {
      taco_set_error("alignment_path: cannot raise the dynamic LDS limit to %zu bytes", kPathLdsBudget);
      return TACO_ELAUNCH;
    }
  } else {
    static DynSmemOnce raised;
    if (!ensure_dyn_smem(raised, reinterpret_cast<const void*>(alignment_path_block_kernel), kPathLdsBudget)) {
      taco_set_error("alignment_path: cannot raise the dynamic LDS limit to %zu bytes", kPathLdsBudget);
      return TACO_ELAUNCH;
    }
    TACO_KLAUNCH(alignment_path_block_kernel, dim3(B), dim3(p.threads), p.lds_bytes, s, alignments, text_length, steps, max_jump, path,
                 dur, counts, mass, path_ws(workspace, B, Td, Tt).way, Td, Tt);
  }
  TACO_LAUNCH_CHECK("alignment_path");
  return TACO_OK;
}
