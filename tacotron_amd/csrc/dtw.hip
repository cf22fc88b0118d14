// dtw.hip -- held-out evaluation on the device (include/taco_hip.h taco_frames_active, taco_frame_dtw, taco_frame_dtw_path): how many
// frames of a padded recording are in use, and the cost of the best dynamic-time-warping path between two frame sequences per batch
// row -- the warp behind mel-cepstral distortion -- with or without the path itself.  No counterpart in the reference, which never
// scores a checkpoint.
//
// frame_dtw: one workgroup per row, one launch.  Cell (i, j) of the Fa x Fb table needs (i-1, j-1), (i-1, j) and (i, j-1) only, so
// the cells of one anti-diagonal d = i + j are independent and need the two diagonals before it: the workgroup walks d = 0 ..
// na + nb - 2 with THREE diagonals of (D, N) in LDS, indexed by i, and the table is never materialised.  One barrier per diagonal is
// enough with three buffers: the buffer written at d + 1 is the one diagonal d read as d - 2, and every wave has passed the barrier
// behind d by then.  No buffer needs initialising: a cell reads predecessors inside the table only, and those were written one or
// two diagonals earlier.
// The coefficients u = basis a_i, v = basis b_j are computed once per row in front of the walk (na K + nb K sums of C products,
// against na nb K products in the walk), with row stride K | 1: the lanes of a wave hold consecutive i (descending j) and read
// u[i][k], v[j][k] for one k at a time, and an odd stride in dwords puts 32 consecutive rows on 32 different banks (K = 13 as it is;
// K = 32 would be 32-way conflicted, 33 is free).  They live in LDS beside the diagonals when both fit 160 KiB -- Fa = Fb = 1024 at
// K = 13 is exactly 128 KiB -- and else in the row's slice of the workspace, which only this workgroup writes and reads (a
// __syncthreads() between the two).
// A diagonal no longer than a wave would need no workgroup barrier; that special case is NOT built: tools/frame_dtw_timing.py
// gives the cost per diagonal it would have to beat.
//
// Arithmetic: the header promises bits a NumPy float32 restatement reproduces, i.e. separately rounded products, sums and
// differences and a correctly rounded square root.  hipcc contracts a * b + c into an FMA by default, and in this toolchain
// __fmul_rn / __fadd_rn are plain operators in a header compiled under that default, so the guarantee is made here instead:
// contraction is switched off for this whole file, and sqrtf is the correctly rounded one (no fast-math flag in build.sh).
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int kDtwThreads = 256;              // 4 waves, one per SIMD: a diagonal of the S1 shape (360 cells) is two passes
constexpr size_t kDtwLdsBudget = 160 * 1024;  // LDS of a CU

__host__ __device__ inline int dtw_stride(int K) { return K | 1; }

struct DtwPlan {
  size_t lds_bytes;       // dynamic LDS of the launch
  bool coef_in_lds;
  int64_t row_floats;     // workspace floats per row (0: none)
};
DtwPlan dtw_plan(int Fa, int Fb, int K) {
  const size_t diag = (size_t)Fa * 3 * (sizeof(float) + sizeof(int32_t));
  const size_t coef = (size_t)(Fa + Fb) * dtw_stride(K) * sizeof(float);
  DtwPlan p;
  p.coef_in_lds = diag + coef <= kDtwLdsBudget;
  p.lds_bytes = p.coef_in_lds ? diag + coef : diag;
  p.row_floats = p.coef_in_lds ? 0 : (int64_t)(Fa + Fb) * dtw_stride(K);
  return p;
}
// The workspace: the B rows' coefficients (none where they fit LDS), and behind them in the path form B direction tables, a byte
// per cell of (Fa + Fb - 1) diagonals x Fa.
__host__ __device__ inline int64_t dtw_way_bytes(int Fa, int Fb) { return (int64_t)(Fa + Fb - 1) * Fa; }
struct DtwWs {
  float* coef;
  uint8_t* way;   // (path form only)
  int64_t bytes;
};
DtwWs dtw_ws(void* ws, int B, int Fa, int Fb, int K, bool path) {
  WsCarver c(ws);
  DtwWs w;
  w.coef = c.take<float>(B * dtw_plan(Fa, Fb, K).row_floats);
  w.way = path ? c.take<uint8_t>(B * dtw_way_bytes(Fa, Fb)) : nullptr;
  w.bytes = c.bytes;
  return w;
}
bool dtw_shape_ok(int B, int Fa, int Fb, int K) {
  return B > 0 && Fa > 0 && Fb > 0 && K > 0 && K <= TACO_DTW_MAX_K && Fa <= TACO_DTW_MAX_FRAMES && Fb <= TACO_DTW_MAX_FRAMES;
}

__device__ __forceinline__ int clamp_len(const int32_t* __restrict__ p, int row, int F) {
  int n = p ? p[row] : F;
  n = n < 0 ? 0 : (n > F ? F : n);
  return __builtin_amdgcn_readfirstlane(n);   // the same for every lane: the walk's trip counts (and its barriers) are uniform
}

// out[i * S + k] = sum_c basis[k, c] x[i, c] for i < n, k < K (basis NULL: x[i, k]).  Item e = i K + k: neighbouring lanes share the
// frame (one broadcast load) and differ in the basis row, which stays in the vector cache (K C floats, 4 KiB at 13 x 80).
__device__ __forceinline__ void dtw_project(const float* __restrict__ x, int n, const float* __restrict__ basis, float* out, int C,
                                            int K, int S) {
  for (int e = threadIdx.x; e < n * K; e += kDtwThreads) {
    const int i = e / K, k = e - i * K;
    const float* xr = x + (int64_t)i * C;
    float acc;
    if (basis) {
      const float* br = basis + k * C;
      acc = 0.f;
      for (int c = 0; c < C; ++c) acc = acc + br[c] * xr[c];   // (two roundings: contraction is off in this file)
    } else {
      acc = xr[k];
    }
    out[i * S + k] = acc;
  }
}

// PATH: every cell also stores which predecessor it took (0: (i-1, j-1), 1: (i-1, j), 2: (i, j-1)) as a byte at way[d * Fa + i],
// d = i + j -- diagonal-major, so the lanes of a wave, which hold consecutive i of one diagonal, store consecutive bytes -- and
// behind the walk the path is read off that table backwards from (na - 1, nb - 1).  `steps` is known by then, so entry steps - 1 - t
// is written directly and nothing is reversed.  The stores are global and nobody waits for them in the walk (lds_barrier() waits
// for LDS only); in front of the backtrack every wave waits for its own (s_waitcnt vmcnt(0)) and then for the others (barrier), and
// the backtrack loads on the vector path past the CU's vector cache (sc1), served by the L2 that acknowledged the stores.
// The cost-only form takes an EMPTY DtwPath behind its twelve arguments and every line of the path form sits under `if constexpr
// (PATH)`: its instructions are those it had before the path form existed (compared in the assembly, kernel by kernel).
template <bool PATH>
struct DtwPath {};
template <>
struct DtwPath<true> {
  int32_t* path_a;     // (B, Fa + Fb - 1)
  int32_t* path_b;
  uint8_t* way;        // B tables of (Fa + Fb - 1) x Fa bytes
};

template <bool COEF_LDS, bool PATH>
__global__ __launch_bounds__(kDtwThreads) void frame_dtw_kernel(const float* __restrict__ a, const int32_t* __restrict__ na_p,
                                                                const float* __restrict__ b, const int32_t* __restrict__ nb_p,
                                                                const float* __restrict__ basis, float* __restrict__ cost,
                                                                int32_t* __restrict__ steps, float* ws, int Fa, int Fb, int C, int K,
                                                                DtwPath<PATH> out) {
  extern __shared__ float dtw_lds[];   // D[3][Fa] | N[3][Fa] | COEF_LDS: U[Fa][S] | V[Fb][S]
  const int row = blockIdx.x, tid = threadIdx.x;
  const int na = clamp_len(na_p, row, Fa), nb = clamp_len(nb_p, row, Fb);
  if (na == 0 || nb == 0) {
    if (tid == 0) cost[row] = 0.f, steps[row] = 0;
    if constexpr (PATH) {
      const int P = Fa + Fb - 1;
      for (int t = tid; t < P; t += kDtwThreads) out.path_a[(int64_t)row * P + t] = -1, out.path_b[(int64_t)row * P + t] = -1;
    }
    return;
  }
  const int S = dtw_stride(K);
  float* D = dtw_lds;
  int32_t* N = reinterpret_cast<int32_t*>(dtw_lds + 3 * Fa);
  float* U = COEF_LDS ? dtw_lds + 6 * Fa : ws + (int64_t)row * (Fa + Fb) * S;
  float* V = U + Fa * S;
  dtw_project(a + (int64_t)row * Fa * C, na, basis, U, C, K, S);
  dtw_project(b + (int64_t)row * Fb * C, nb, basis, V, C, K, S);
  __syncthreads();   // (also orders the workspace form's global stores in front of this workgroup's loads)
  uint8_t* way = nullptr;
  if constexpr (PATH) way = out.way + row * dtw_way_bytes(Fa, Fb);

  const int last = na + nb - 2;
  for (int d = 0; d <= last; ++d) {
    const int ilo = d - (nb - 1) > 0 ? d - (nb - 1) : 0, ihi = d < na - 1 ? d : na - 1;
    const int c0 = (d % 3) * Fa, c1 = ((d + 2) % 3) * Fa, c2 = ((d + 1) % 3) * Fa;   // this diagonal, d - 1, d - 2
    for (int i = ilo + tid; i <= ihi; i += kDtwThreads) {
      const int j = d - i;
      // the three candidates, loaded whether they exist or not (the index stays inside the buffers; a value that is not a cell of
      // the table is never selected) so that all six reads are in flight together with the coefficients'
      const int im = i > 0 ? i - 1 : 0;
      const float d_diag = D[c2 + im], d_up = D[c1 + im], d_left = D[c1 + i];
      const int n_diag = N[c2 + im], n_up = N[c1 + im], n_left = N[c1 + i];
      const float* u = U + i * S;
      const float* v = V + j * S;
      float s = 0.f;
#pragma unroll 4   // (four pairs of LDS reads in flight per wait; the sum keeps its order)
      for (int k = 0; k < K; ++k) {
        const float t = u[k] - v[k];
        s = s + t * t;
      }
      float best = sqrtf(s);
      int count = 1;
      uint8_t took = 0;
      if (d > 0) {
        // in the order (i-1, j-1), (i-1, j), (i, j-1); a later candidate replaces an earlier one only when strictly smaller
        const bool has_up = i > 0, has_left = j > 0;
        bool have = has_up && has_left;
        float pd = d_diag;
        int pn = n_diag;
        const bool take_up = has_up && (!have || d_up < pd);
        pd = take_up ? d_up : pd, pn = take_up ? n_up : pn, have = have || has_up;
        const bool take_left = has_left && (!have || d_left < pd);
        pd = take_left ? d_left : pd, pn = take_left ? n_left : pn;
        best = pd + best;
        count = pn + 1;
        if constexpr (PATH) took = take_left ? 2 : (take_up ? 1 : 0);
      }
      D[c0 + i] = best;
      N[c0 + i] = count;
      if constexpr (PATH) way[d * Fa + i] = took;
      if (d == last) cost[row] = best, steps[row] = count;   // (the last diagonal is the one cell (na - 1, nb - 1))
    }
    lds_barrier();
  }
  if constexpr (PATH) {
    // every wave's direction stores are acknowledged before any lane reads the table.  The wait is written out: at workgroup
    // scope hipcc's __syncthreads() waits for lgkmcnt only on this target (stores and plain loads of one CU meet in its vector
    // cache), and the loads below do not go through that cache
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int P = Fa + Fb - 1;
    int32_t* path_a = out.path_a + (int64_t)row * P;
    int32_t* path_b = out.path_b + (int64_t)row * P;
    int n = N[(last % 3) * Fa + na - 1];   // steps[row]
    n = n < 0 ? 0 : (n > P ? P : n);       // (it is in 1 .. P; the bounds of the stores below do not rest on the data)
    for (int t = n + tid; t < P; t += kDtwThreads) path_a[t] = -1, path_b[t] = -1;
    if (tid == 0) {   // one dependent load per step: tools/frame_dtw_path_timing.py has what the chain costs
      int i = na - 1, j = nb - 1;
      for (int t = n - 1; t >= 0; --t) {
        path_a[t] = i, path_b[t] = j;
        if (t == 0) break;
        const unsigned w = __hip_atomic_load(way + (i + j) * Fa + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        i = (w != 2 && i > 0) ? i - 1 : i;
        j = (w != 1 && j > 0) ? j - 1 : j;
      }
    }
  }
}

// n[b] = 1 + the last frame with an element above `floor`.  A workgroup per row, every element read once, coalesced; the per-thread
// maxima meet in one LDS word (a maximum: no order dependence).
__global__ __launch_bounds__(256) void frames_active_kernel(const float* __restrict__ x, float floor, int32_t* __restrict__ n, int F,
                                                            int C) {
  __shared__ int last;
  if (threadIdx.x == 0) last = -1;
  __syncthreads();
  const float* xr = x + (int64_t)blockIdx.x * F * C;
  const int64_t total = (int64_t)F * C;
  int mine = -1;
  for (int64_t e = threadIdx.x; e < total; e += 256)
    if (xr[e] > floor) mine = (int)(e / C);   // (e ascends: the last hit of a thread is its largest frame; false for a NaN)
  if (mine >= 0) atomicMax(&last, mine);
  __syncthreads();
  if (threadIdx.x == 0) n[blockIdx.x] = last + 1;
}

}  // namespace

int launch_frames_active(const float* x, float floor, int32_t* n, int B, int F, int C, hipStream_t s) {
  TACO_KLAUNCH(frames_active_kernel, dim3(B), dim3(256), 0, s, x, floor, n, F, C);
  TACO_LAUNCH_CHECK("frames_active");
  return TACO_OK;
}

int launch_frame_dtw(const float* a, const int32_t* na, const float* b, const int32_t* nb, const float* basis, float* cost, int32_t* steps,
                     float* workspace, int B, int Fa, int Fb, int C, int K, hipStream_t s) {
  const DtwPlan p = dtw_plan(Fa, Fb, K);
  static DynSmemOnce raised;
  const auto in_lds = frame_dtw_kernel<true, false>, in_ws = frame_dtw_kernel<false, false>;
  if (p.coef_in_lds) {   // up to the whole budget, raised once per device for every later shape
    if (!ensure_dyn_smem(raised, reinterpret_cast<const void*>(in_lds), kDtwLdsBudget)) {
      taco_set_error("frame_dtw: cannot raise the dynamic LDS limit to %zu bytes", kDtwLdsBudget);
      return TACO_ELAUNCH;
    }
    TACO_KLAUNCH(in_lds, dim3(B), dim3(kDtwThreads), p.lds_bytes, s, a, na, b, nb, basis, cost, steps, workspace, Fa, Fb, C, K,
                 DtwPath<false>{});
  } else {               // the diagonals alone: 24 KiB at the most
    TACO_KLAUNCH(in_ws, dim3(B), dim3(kDtwThreads), p.lds_bytes, s, a, na, b, nb, basis, cost, steps, workspace, Fa, Fb, C, K,
                 DtwPath<false>{});
  }
  TACO_LAUNCH_CHECK("frame_dtw");
  return TACO_OK;
}

int launch_frame_dtw_path(const float* a, const int32_t* na, const float* b, const int32_t* nb, const float* basis, float* cost,
                          int32_t* steps, int32_t* path_a, int32_t* path_b, void* workspace, int B, int Fa, int Fb, int C, int K,
                          hipStream_t s) {
  const DtwPlan p = dtw_plan(Fa, Fb, K);
  const DtwWs w = dtw_ws(workspace, B, Fa, Fb, K, true);
  float* coef = w.coef;
  const DtwPath<true> out = {path_a, path_b, w.way};
  static DynSmemOnce raised;
  const auto in_lds = frame_dtw_kernel<true, true>, in_ws = frame_dtw_kernel<false, true>;
  if (p.coef_in_lds) {
    if (!ensure_dyn_smem(raised, reinterpret_cast<const void*>(in_lds), kDtwLdsBudget)) {
      taco_set_error("frame_dtw_path: cannot raise the dynamic LDS limit to %zu bytes", kDtwLdsBudget);
      return TACO_ELAUNCH;
    }
    TACO_KLAUNCH(in_lds, dim3(B), dim3(kDtwThreads), p.lds_bytes, s, a, na, b, nb, basis, cost, steps, coef, Fa, Fb, C, K, out);
  } else {
    TACO_KLAUNCH(in_ws, dim3(B), dim3(kDtwThreads), p.lds_bytes, s, a, na, b, nb, basis, cost, steps, coef, Fa, Fb, C, K, out);
  }
  TACO_LAUNCH_CHECK("frame_dtw_path");
  return TACO_OK;
}

extern "C" int taco_frames_active(const float* x, float floor, int32_t* n, int B, int F, int C, void* stream) {
  TACO_REQUIRE(x, "frames_active: x is NULL");
  TACO_REQUIRE(n, "frames_active: n is NULL");
  TACO_REQUIRE(B > 0, "frames_active: B=%d must be positive", B);
  TACO_REQUIRE(F > 0, "frames_active: F=%d must be positive", F);
  TACO_REQUIRE(C > 0, "frames_active: C=%d must be positive", C);
  return launch_frames_active(x, floor, n, B, F, C, as_stream(stream));
}

// What taco_frame_dtw and taco_frame_dtw_path both require, in the order a caller sees the refusals.  `who`: the entry point's name
// in the messages; missing: what that entry point alone needs and did not get (refused behind the shared operands), or nullptr.
static int dtw_require(const char* who, const void* a, const void* b, const void* cost, const void* steps, const char* missing,
                       const void* basis, int B, int Fa, int Fb, int C, int K) {
  TACO_REQUIRE(a, "%s: a is NULL", who);
  TACO_REQUIRE(b, "%s: b is NULL", who);
  TACO_REQUIRE(cost, "%s: cost is NULL", who);
  TACO_REQUIRE(steps, "%s: steps is NULL", who);
  TACO_REQUIRE(!missing, "%s: %s", who, missing);
  TACO_REQUIRE(B > 0, "%s: B=%d must be positive", who, B);
  TACO_REQUIRE(Fa > 0 && Fb > 0, "%s: Fa=%d and Fb=%d must be positive", who, Fa, Fb);
  TACO_REQUIRE(C > 0 && K > 0, "%s: C=%d and K=%d must be positive", who, C, K);
  TACO_REQUIRE(basis || K == C, "%s: without a basis K=%d must equal C=%d", who, K, C);
  TACO_REQUIRE(K <= TACO_DTW_MAX_K, "%s: K=%d is above the %d coefficients a frame may have", who, K, TACO_DTW_MAX_K);
  TACO_REQUIRE(C <= TACO_DTW_MAX_C, "%s: C=%d is above the %d channels a frame may have", who, C, TACO_DTW_MAX_C);
  TACO_REQUIRE(Fa <= TACO_DTW_MAX_FRAMES && Fb <= TACO_DTW_MAX_FRAMES, "%s: Fa=%d or Fb=%d is above the %d frames a row may have", who, Fa,
               Fb, TACO_DTW_MAX_FRAMES);
  return TACO_OK;
}

extern "C" int64_t taco_frame_dtw_workspace_bytes(int B, int Fa, int Fb, int K) {
  if (!dtw_shape_ok(B, Fa, Fb, K)) return TACO_EINVAL;
  return dtw_ws(nullptr, B, Fa, Fb, K, false).bytes;
}

extern "C" int taco_frame_dtw(const float* a, const int32_t* na, const float* b, const int32_t* nb, const float* basis, float* cost,
                              int32_t* steps, void* workspace, int B, int Fa, int Fb, int C, int K, void* stream) {
  TACO_TRY(dtw_require("frame_dtw", a, b, cost, steps, nullptr, basis, B, Fa, Fb, C, K));
  TACO_REQUIRE(workspace || dtw_plan(Fa, Fb, K).row_floats == 0, "frame_dtw: workspace is NULL and Fa=%d, Fb=%d, K=%d need one", Fa, Fb, K);
  return launch_frame_dtw(a, na, b, nb, basis, cost, steps, dtw_ws(workspace, B, Fa, Fb, K, false).coef, B, Fa, Fb, C, K,
                          as_stream(stream));
}

extern "C" int64_t taco_frame_dtw_path_workspace_bytes(int B, int Fa, int Fb, int K) {
  if (!dtw_shape_ok(B, Fa, Fb, K)) return TACO_EINVAL;
  return dtw_ws(nullptr, B, Fa, Fb, K, true).bytes;
}

extern "C" int taco_frame_dtw_path(const float* a, const int32_t* na, const float* b, const int32_t* nb, const float* basis, float* cost,
                                   int32_t* steps, int32_t* path_a, int32_t* path_b, void* workspace, int B, int Fa, int Fb, int C, int K,
                                   void* stream) {
  const char* missing = !path_a      ? "path_a is NULL"
                        : !path_b    ? "path_b is NULL"
                        : !workspace ? "workspace is NULL (the direction table lives there)"
                                     : nullptr;
  TACO_TRY(dtw_require("frame_dtw_path", a, b, cost, steps, missing, basis, B, Fa, Fb, C, K));
  return launch_frame_dtw_path(a, na, b, nb, basis, cost, steps, path_a, path_b, workspace, B, Fa, Fb, C, K,
                               as_stream(stream));
}
