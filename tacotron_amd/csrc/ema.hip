// ema.hip -- exponential moving average of the flat parameter buffer (include/taco_hip.h taco_param_ema and its size function).  The
// reference has no weight averaging; this is tf.train.ExponentialMovingAverage's update, `shadow -= (1 - decay) (shadow - var)`,
// as one pass behind the clip + Adam update on the step's stream.
//
// Every value is a single rounded fp32 operation in a stated order (no contraction): d = p - e, t = w d, e' = e + t, so the result
// is the same bits as the NumPy float32 restatement tests/ema_ref.py.  The weight w = 1 - decay_k comes from the host; the kernel
// holds no schedule.
//   ema_kernel<VEC, STATS>  grid-stride over the buffer: 16-byte loads and stores when both pointers are 16-byte aligned (VEC; four
//                           groups of a thread in flight, the n % 4 floats behind the last whole group by workgroup 0), else float by
//                           float.  STATS: every thread adds (double)d^2 and (double)p^2 in the order it meets them (the squares of
//                           fp32 values are exact in fp64: only the sums round); the lanes of a wave meet in a fixed tree, the waves
//                           in sequence -> one pair of partials per workgroup in the workspace.  The bits of ema do not depend on
//                           STATS: the same three operations either way
//   ema_fold_kernel         one workgroup: partial b goes to thread b mod 256 in increasing b, then the same tree -> stats[0..3)
// The guard is taco_clip_adam_step_guarded's: with either error word set, ema_kernel returns before it reads or writes anything and
// the fold writes (-1, -1, 0) without reading the workspace.  No atomics; the grid follows from n and the device's CU count alone, so
// the same call on the same inputs gives the same bits.  Every partial the fold reads was written by the launch in front of it.
#include <math.h>

#include "kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int EM_T = 256, EM_NW = EM_T / 64;
constexpr int EM_MAX_BLOCKS = 4096;   // what the workspace holds partials for, whatever the device
constexpr int EM_BLOCKS_PER_CU = 8;   // 2048 threads per CU: every wave slot of it
constexpr int EM_BATCH = 4;           // 16-byte groups of either operand a thread has in flight

// One rounded fp32 operation each: plain operators under this file's `fp contract(off)` (limiter.hip says why not __fmul_rn)
__device__ __forceinline__ float em_update(float e, float p, float w, float& d) {
  d = p - e;
  const float t = w * d;
  return e + t;
}

struct EmAcc { double d2 = 0.0, p2 = 0.0; };

template <bool STATS>
__device__ __forceinline__ float em_one(float e, float p, float w, EmAcc& a) {
  float d;
  const float r = em_update(e, p, w, d);
  if (STATS) {
    const double dd = (double)d, pd = (double)p;
    a.d2 = fma(dd, dd, a.d2);   // the square of an fp32 value is exact in fp64: one rounding, that of the sum
    a.p2 = fma(pd, pd, a.p2);
  }
  return r;
}

template <bool STATS>
__device__ __forceinline__ float4 em_four(float4 e, float4 p, float w, EmAcc& a) {
  float4 r;
  r.x = em_one<STATS>(e.x, p.x, w, a);
  r.y = em_one<STATS>(e.y, p.y, w, a);
  r.z = em_one<STATS>(e.z, p.z, w, a);
  r.w = em_one<STATS>(e.w, p.w, w, a);
  return r;
}

// v_l += v_(l + 32), then + 16, 8, 4, 2, 1; lane 0 holds the total
__device__ __forceinline__ double em_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_down(v, o);
  return v;
}

// lane 0 of every wave has its wave's pair; thread 0 adds the waves in sequence and returns the workgroup's pair
__device__ __forceinline__ bool em_block_sum(EmAcc& a, double (*red)[EM_NW]) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  a.d2 = em_wave_sum(a.d2);
  a.p2 = em_wave_sum(a.p2);
  if (lane == 0) {
    red[0][wv] = a.d2;
    red[1][wv] = a.p2;
  }
  __syncthreads();
  if (threadIdx.x != 0) return false;
  for (int k = 1; k < EM_NW; ++k) {
    a.d2 = a.d2 + red[0][k];
    a.p2 = a.p2 + red[1][k];
  }
  return true;
}

template <bool VEC, bool STATS>
__global__ __launch_bounds__(EM_T) void ema_kernel(float* __restrict__ ema, const float* __restrict__ params, int64_t n, float w,
                                                   const int32_t* __restrict__ err, double* __restrict__ part) {
  __shared__ double red[2][EM_NW];
  if (err && (err[0] | err[1])) return;   // (the whole grid: a skipped Adam update is not averaged in)
  EmAcc a;
  const int64_t stride = (int64_t)gridDim.x * EM_T;
  int64_t i = (int64_t)blockIdx.x * EM_T + threadIdx.x;
  if (VEC) {
    const int64_t n4 = n / 4;
    float4* e4 = reinterpret_cast<float4*>(ema);
    const float4* p4 = reinterpret_cast<const float4*>(params);
    for (; i + (EM_BATCH - 1) * stride < n4; i += EM_BATCH * stride) {
      float4 e[EM_BATCH], p[EM_BATCH];
#pragma unroll
      for (int k = 0; k < EM_BATCH; ++k) {
        e[k] = e4[i + k * stride];
        p[k] = p4[i + k * stride];
      }
#pragma unroll
      for (int k = 0; k < EM_BATCH; ++k) e4[i + k * stride] = em_four<STATS>(e[k], p[k], w, a);
    }
    for (; i < n4; i += stride) e4[i] = em_four<STATS>(e4[i], p4[i], w, a);
    const int64_t j = n4 * 4 + threadIdx.x;   // the n % 4 floats behind the last whole group
    if (blockIdx.x == 0 && threadIdx.x < 4 && j < n) ema[j] = em_one<STATS>(ema[j], params[j], w, a);
  } else {
    for (; i < n; i += stride) ema[i] = em_one<STATS>(ema[i], params[i], w, a);
  }
  if (STATS && em_block_sum(a, red)) {
    part[2 * blockIdx.x] = a.d2;
    part[2 * blockIdx.x + 1] = a.p2;
  }
}

__global__ __launch_bounds__(EM_T) void ema_fold_kernel(const double* __restrict__ part, int blocks, const int32_t* __restrict__ err,
                                                        double* __restrict__ stats) {
  __shared__ double red[2][EM_NW];
  if (err && (err[0] | err[1])) {   // (uniform) the workspace was not written: it is not read
    if (threadIdx.x == 0) {
      stats[0] = -1.0;
      stats[1] = -1.0;
      stats[2] = 0.0;
    }
    return;
  }
  EmAcc a;
  for (int b = threadIdx.x; b < blocks; b += EM_T) {
    a.d2 = a.d2 + part[2 * b];
    a.p2 = a.p2 + part[2 * b + 1];
  }
  if (!em_block_sum(a, red)) return;
  stats[0] = a.d2;
  stats[1] = a.p2;
  stats[2] = 1.0;
}

// workgroups of ema_kernel: enough for every element at one group (VEC) or float per thread and batch, at most EM_BLOCKS_PER_CU
// per CU of the current device and never more than the workspace holds partials for
int em_grid(int64_t n, bool vec) {
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (cus < 1) cus = 256;
  const int64_t per_block = vec ? (int64_t)EM_T * 4 * EM_BATCH : EM_T;
  int64_t g = (n + per_block - 1) / per_block;
  const int64_t cap = (int64_t)cus * EM_BLOCKS_PER_CU < EM_MAX_BLOCKS ? (int64_t)cus * EM_BLOCKS_PER_CU : EM_MAX_BLOCKS;
  if (g > cap) g = cap;
  return g < 1 ? 1 : (int)g;
}

// workspace of taco_param_ema: one pair of fp64 partials per workgroup the call can launch, on any device.  No slack: a base that
// is not 8-byte aligned is refused.
struct EmWs {
  double* part;
  int64_t bytes;
};
EmWs em_ws(void* ws) {
  WsCarver c(ws);
  EmWs w;
  w.part = c.take<double>((int64_t)EM_MAX_BLOCKS * 2);
  w.bytes = c.bytes;
  return w;
}

}  // namespace

extern "C" int64_t taco_param_ema_workspace_bytes(int64_t n) {
  if (n <= 0) return TACO_EINVAL;
  return em_ws(nullptr).bytes;
}

extern "C" int taco_param_ema(float* ema, const float* params, int64_t n, float w, const int32_t* err_words, double* stats,
                              void* workspace, void* stream) {
  TACO_REQUIRE(ema && params, "param_ema: ema or params is NULL");
  TACO_REQUIRE(n > 0, "param_ema: n=%lld must be positive", (long long)n);
  TACO_REQUIRE(w >= 0.f && w <= 1.f, "param_ema: w=%g is not in [0, 1]", (double)w);   // (NaN fails both)
  TACO_REQUIRE(!bytes_meet(ema, (uint64_t)n * sizeof(float), params, (uint64_t)n * sizeof(float)), "param_ema: ema may not overlap params");
  TACO_REQUIRE(!stats || workspace, "param_ema: stats given without a workspace");
  TACO_REQUIRE(!stats || ((reinterpret_cast<uintptr_t>(stats) & 7) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0),
               "param_ema: stats or workspace is not 8-byte aligned");
  hipStream_t s = as_stream(stream);
  const bool vec = ((reinterpret_cast<uintptr_t>(ema) | reinterpret_cast<uintptr_t>(params)) & 15) == 0;
  const int grid = em_grid(n, vec);
  double* part = em_ws(workspace).part;   // (null without a workspace: only the stats forms read it)
  if (stats) {
    if (vec) TACO_KLAUNCH((ema_kernel<true, true>), dim3(grid), dim3(EM_T), 0, s, ema, params, n, w, err_words, part);
    else TACO_KLAUNCH((ema_kernel<false, true>), dim3(grid), dim3(EM_T), 0, s, ema, params, n, w, err_words, part);
    TACO_KLAUNCH(ema_fold_kernel, dim3(1), dim3(EM_T), 0, s, part, grid, err_words, stats);
  } else {
    if (vec) TACO_KLAUNCH((ema_kernel<true, false>), dim3(grid), dim3(EM_T), 0, s, ema, params, n, w, err_words, (double*)nullptr);
    else TACO_KLAUNCH((ema_kernel<false, false>), dim3(grid), dim3(EM_T), 0, s, ema, params, n, w, err_words, (double*)nullptr);
  }
  TACO_LAUNCH_CHECK("param_ema");
  return TACO_OK;
}
