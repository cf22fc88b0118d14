// loudness.hip -- ITU-R BS.1770 integrated loudness of finished waveforms and a gain to a target level (include/taco_hip.h
// taco_k_weighting, taco_wave_loudness).  No counterpart in the reference, which writes whatever level the checkpoint produced.
//
// The K-weighting is two biquads in cascade, each in the transposed direct form II, so a row's filter state is four floats
// S = (s1, s2, t1, t2) and one sample is the affine map S -> M S + v x with a CONSTANT 4 x 4 matrix M (block lower triangular: the
// shelf does not see the high-pass).  A run of k samples therefore is S -> M^k S + R with R the run's end state from a zero state,
// and M^k depends on k alone: the host forms M^8, M^16, ..., M^512 and M^2048, ..., M^65536 in fp64 by repeated squaring and hands them
// to the kernels.  A row is cut into chunks of WL_CHUNK = 2048 samples at FIXED positions (chunk c = samples [2048 c, 2048 c + 2048) of
// the row, whatever B and L are), one workgroup per chunk, a thread owns 8 consecutive samples:
//   wl_filter<true>   the chunk's end state from a zero carry, into the workspace (only chunks that have a successor)
//   wl_carry          one wave per row: the state that enters every chunk, by the same lane scan over the chunks' end states with
//                     M^2048, M^4096, ..., M^65536, 64 chunks at a time (rows of more than one chunk only)
//   wl_filter<false>  the state that enters every thread's run from the chunk's carry, the run again FROM that state (no
//                     per-sample correction terms: the second pass is the recursion itself), y into the workspace and max |x|
//                     of the chunk
// WHERE THE PRECISION GOES.  The high-pass has a double pole at radius 0.985 (16 kHz) to 0.995 (48 kHz): sum_k M^(8 k) is of the
// order of 1 / (1 - r^8)^2 = 650 at 48 kHz, and under a constant input every thread's run from a zero state is the SAME numbers, so
// its rounding error is the same in every thread and the scan multiplies it by that sum instead of averaging it out.  With the
// zero-state runs and the scan in fp32 a DC step of 0.5 at 48 kHz left 1.2e-3 of residue in y and read 0.0156 LU high -- with fp64
// combines as well, so it is the runs, not the products (profiles/wave_loudness_forms.txt).  Hence: the runs from a zero state, the
// scan and every carry are fp64 (8 samples x 10 fused multiply-adds per thread, twice per call); the state that enters a thread's run is
// rounded to fp32 once, and the second run, the one that yields y, is fp32: its rounding errors cannot accumulate beyond 8 samples.
//   wl_hops           h_k = sum of y^2 over hop k (one wave per hop; a row shorter than four hops is one "hop" of n_b samples)
//   wl_gates          one workgroup per row: blocks, the two gates, I, M, the peak, the gain -> loud, blocks
//   wl_emit<T>        out = x g / pcm, 16-byte / 8-byte stores at any row alignment (wj_pcm_kernel's form), zeros behind n_b
// No workgroup waits for another one inside a launch; the order of every sum depends on the position in the row and n_b alone.
#include <math.h>

#include <algorithm>

#include "kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int WL_T = 256, WL_PER = 8, WL_CHUNK = WL_T * WL_PER;
constexpr int WL_NW = WL_T / 64;
constexpr int WL_GT = 256;   // wl_gates block
constexpr int WL_ET = 256, WL_EPER = 4;
static_assert(WL_CHUNK == TACO_LOUD_CHUNK, "include/taco_hip.h states the chunk length");

// rows of a power of M: (s1', s2') = A (s1, s2), (t1', t2') = C (s1, s2) + D (t1, t2)
struct WlMat {
  double a[4], c[4], d[4];
};
template <typename T>
struct WlCoef {
  T sb0, sb1, sb2, sa1, sa2;   // the shelf, rounded once to fp32 (T = double: those values, widened)
  T ha1, ha2;                  // the high-pass (b = 1, -2, 1)
};
struct WlParams {
  WlCoef<float> f;
  WlCoef<double> d;
  WlMat lane[6];                   // M^(8 d), d = 1, 2, 4, 8, 16, 32: the scan across the lanes of a wave
  WlMat run;                       // M^8: a thread's run
  WlMat wave;                      // M^512
};
struct WlCarryParams {
  WlMat lane[6];                   // M^(2048 d), d = 1, 2, 4, 8, 16, 32: the scan across the chunks of a row
};
template <typename T>
struct WlStateT {
  T s1, s2, t1, t2;
};
using WlState = WlStateT<double>;   // the scan's

__device__ __forceinline__ int wl_len(const int32_t* __restrict__ samples, int b, int L) {
  if (!samples) return L;
  const int n = samples[b];
  return n < 0 ? 0 : (n > L ? L : n);
}

// one sample through both biquads (transposed direct form II): u = shelf(x), y = highpass(u)
__device__ __forceinline__ float wl_fma(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double wl_fma(double a, double b, double c) { return fma(a, b, c); }
template <typename T>
__device__ __forceinline__ T wl_step(const WlCoef<T>& p, WlStateT<T>& s, T x) {
  const T u = wl_fma(p.sb0, x, s.s1);
  s.s1 = wl_fma(-p.sa1, u, wl_fma(p.sb1, x, s.s2));
  s.s2 = wl_fma(-p.sa2, u, p.sb2 * x);
  const T y = u + s.t1;
  s.t1 = wl_fma(-p.ha1, y, wl_fma((T)-2, u, s.t2));
  s.t2 = wl_fma(-p.ha2, y, u);
  return y;
}

// x + m p: the state p seen through a power of M, added to x
__device__ __forceinline__ WlState wl_madd(const WlMat& m, const WlState& p, const WlState& x) {
  WlState r;
  r.s1 = fma(m.a[0], p.s1, fma(m.a[1], p.s2, x.s1));
  r.s2 = fma(m.a[2], p.s1, fma(m.a[3], p.s2, x.s2));
  // (the high-pass terms outermost: in a chain of these products the way from p.t to r.t is two fused multiply-adds, not four)
  r.t1 = fma(m.d[0], p.t1, fma(m.d[1], p.t2, fma(m.c[0], p.s1, fma(m.c[1], p.s2, x.t1))));
  r.t2 = fma(m.d[2], p.t1, fma(m.d[3], p.t2, fma(m.c[2], p.s1, fma(m.c[3], p.s2, x.t2))));
  return r;
}

__device__ __forceinline__ WlState wl_shfl_up(const WlState& s, int d) {
  WlState r;
  r.s1 = __shfl_up(s.s1, d);
  r.s2 = __shfl_up(s.s2, d);
  r.t1 = __shfl_up(s.t1, d);
  r.t2 = __shfl_up(s.t2, d);
  return r;
}

// inclusive scan over the lanes of a wave: lane l ends with sum_{u <= l} M^(8 (l - u)) r_u
__device__ __forceinline__ WlState wl_wave_scan(const WlMat (&pw)[6], WlState r, int lane) {
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int d = 1 << k;
    const WlState prev = wl_shfl_up(r, d);
    if (lane >= d) r = wl_madd(pw[k], prev, r);
  }
  return r;
}

__device__ __forceinline__ WlState wl_load(const double* g) {
  const double2 g0 = *reinterpret_cast<const double2*>(g), g1 = *reinterpret_cast<const double2*>(g + 2);
  return {g0.x, g0.y, g1.x, g1.y};
}
__device__ __forceinline__ void wl_store(double* g, const WlState& e) {
  *reinterpret_cast<double2*>(g) = make_double2(e.s1, e.s2);
  *reinterpret_cast<double2*>(g + 2) = make_double2(e.t1, e.t2);
}

// agg[b, c] (the end state of chunk c from a zero carry, chunks with a successor) -> carry[b, c] = the state that enters chunk c, for
// every chunk of the row but the first, whose carry is zero and is not stored.  One wave per row, lane l the chunk c0 + l of a tile
// of 64: the state at the end of chunk c0 is its aggregate plus M^2048 times the state that entered it, the lane scan carries that on,
// and what enters chunk c + 1 is the scanned value of chunk c
__global__ __launch_bounds__(64) void wl_carry_kernel(const double* __restrict__ agg_all, double* __restrict__ carry_all,
                                                      const int32_t* __restrict__ samples, const WlCarryParams q, int nch, int L) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int n = wl_len(samples, b, L);
  const int nc = (int)(((int64_t)n + WL_CHUNK - 1) / WL_CHUNK);   // chunks in use: aggregates exist for 0 .. nc - 2
  const double* agg = agg_all + (int64_t)b * nch * 4;
  double* carry = carry_all + (int64_t)b * nch * 4;
  WlState run = {0.0, 0.0, 0.0, 0.0};   // the state that enters the tile's first chunk
  for (int c0 = 0; c0 < nc - 1; c0 += 64) {   // (uniform)
    const int c = c0 + lane;
    WlState a = {0.0, 0.0, 0.0, 0.0};
    if (c < nc - 1) a = wl_load(agg + 4 * (int64_t)c);
    if (lane == 0) a = wl_madd(q.lane[0], run, a);
    a = wl_wave_scan(q.lane, a, lane);   // the state at the end of chunk c
    // (a lane's scanned value holds nothing of the lanes behind it: the zeros of chunks past the row's end reach no stored value)
    if (c + 1 < nc) wl_store(carry + 4 * (int64_t)(c + 1), a);
    run.s1 = __shfl(a.s1, 63);
    run.s2 = __shfl(a.s2, 63);
    run.t1 = __shfl(a.t1, 63);
    run.t2 = __shfl(a.t2, 63);
  }
}

template <bool AGG>
__global__ __launch_bounds__(WL_T) void wl_filter_kernel(const float* __restrict__ wave, const int32_t* __restrict__ samples,
                                                         const WlParams p, float* __restrict__ y_all, int64_t y_pitch,
                                                         double* __restrict__ agg_all, int nch, float* __restrict__ cmax_all, int L) {
  __shared__ WlState sh[WL_NW];
  __shared__ float shm[WL_NW];
  const int c = blockIdx.x, b = blockIdx.y;
  const int n = wl_len(samples, b, L);
  const int64_t base = (int64_t)c * WL_CHUNK;
  if (AGG ? base + WL_CHUNK >= n : base >= n) return;   // (the whole workgroup) AGG: nobody reads the last chunk's aggregate
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const float* x = wave + (int64_t)b * L;
  const int64_t i0 = base + (int64_t)threadIdx.x * WL_PER;
  float v[WL_PER];
  if (i0 + WL_PER <= n && (reinterpret_cast<uintptr_t>(x + i0) & 15) == 0) {
    const float4 q0 = *reinterpret_cast<const float4*>(x + i0), q1 = *reinterpret_cast<const float4*>(x + i0 + 4);
    v[0] = q0.x; v[1] = q0.y; v[2] = q0.z; v[3] = q0.w;
    v[4] = q1.x; v[5] = q1.y; v[6] = q1.z; v[7] = q1.w;
  } else {
#pragma unroll
    for (int j = 0; j < WL_PER; ++j) v[j] = i0 + j < n ? x[i0 + j] : 0.f;   // (samples from n_b on are never read)
  }
  // the thread's run from a zero state (fp64)
  WlState r = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int j = 0; j < WL_PER; ++j) (void)wl_step(p.d, r, (double)v[j]);
  // the waves' end states from a zero state at the wave's start
  const WlState inc = wl_wave_scan(p.lane, r, lane);
  if (lane == 63) sh[w] = inc;
  __syncthreads();
  if (AGG) {
    if (threadIdx.x == 0) {
      WlState e = sh[0];
      for (int k = 1; k < WL_NW; ++k) e = wl_madd(p.wave, e, sh[k]);
      wl_store(agg_all + ((int64_t)b * nch + c) * 4, e);
    }
    return;
  }
  // the state that enters the chunk, then the one that enters this wave
  WlState carry = {0.0, 0.0, 0.0, 0.0};
  if (c > 0) carry = wl_load(agg_all + ((int64_t)b * nch + c) * 4);   // (uniform) this launch is handed wl_carry_kernel's array
  for (int k = 0; k < w; ++k) carry = wl_madd(p.wave, carry, sh[k]);
  // lane 0's run ends at r + M^8 carry; the scan again then carries it to every lane.  The state that enters a thread's run is the
  // inclusive value of the lane in front (the carry itself for lane 0)
  if (lane == 0) r = wl_madd(p.run, carry, r);
  const WlState inc2 = wl_wave_scan(p.lane, r, lane);
  WlState e = wl_shfl_up(inc2, 1);
  if (lane == 0) e = carry;
  WlStateT<float> ef = {(float)e.s1, (float)e.s2, (float)e.t1, (float)e.t2};   // rounded once; the run that yields y is fp32
  float y[WL_PER];
#pragma unroll
  for (int j = 0; j < WL_PER; ++j) y[j] = wl_step(p.f, ef, v[j]);
  float* yo = y_all + (int64_t)b * y_pitch + i0;   // (16-byte aligned: the pitch is a multiple of 4 floats, i0 of 8)
  float m = 0.f;
  if (i0 + WL_PER <= n) {
    *reinterpret_cast<float4*>(yo) = make_float4(y[0], y[1], y[2], y[3]);
    *reinterpret_cast<float4*>(yo + 4) = make_float4(y[4], y[5], y[6], y[7]);
#pragma unroll
    for (int j = 0; j < WL_PER; ++j) m = fmaxf(m, fabsf(v[j]));
  } else {
#pragma unroll
    for (int j = 0; j < WL_PER; ++j)
      if (i0 + j < n) {
        yo[j] = y[j];
        m = fmaxf(m, fabsf(v[j]));
      }
  }
  m = wave_max(m);
  if (lane == 0) shm[w] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < WL_NW; ++k) m = fmaxf(m, shm[k]);
    cmax_all[(int64_t)b * nch + c] = m;
  }
}

// h[b, k] = sum of y^2 over hop k: lane l adds the rounded squares of samples l, l + 64, ... of the hop in that order, then the
// lanes' sums meet in wave_sum's fixed tree.  A row shorter than four hops has one "hop": all of its n_b samples
__global__ __launch_bounds__(WL_T) void wl_hops_kernel(const float* __restrict__ y_all, int64_t y_pitch, const int32_t* __restrict__ samples,
                                                       float* __restrict__ h_all, int nhmax, int H, int L) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int n = wl_len(samples, b, L);
  const int k = blockIdx.x * WL_NW + (threadIdx.x >> 6);
  const int nh = n / H;
  int64_t lo, len;
  if (nh >= 4) {
    if (k >= nh) return;
    lo = (int64_t)k * H;
    len = H;
  } else {
    if (k > 0 || n == 0) return;
    lo = 0;
    len = n;
  }
  const float* y = y_all + (int64_t)b * y_pitch + lo;
  float acc = 0.f;
  for (int64_t i = lane; i < len; i += 64) {
    const float t = y[i];
    acc = __fadd_rn(acc, __fmul_rn(t, t));
  }
  acc = wave_sum(acc);
  if (lane == 0) h_all[(int64_t)b * nhmax + k] = acc;
}

// the sum of one float and one count per thread over the workgroup: wave_sum's tree, then the waves in order.  Every thread gets both
__device__ __forceinline__ void wl_block_sum(float& s, int& n, float* shs, int* shn) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  s = wave_sum(s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
  __syncthreads();   // (the arrays may still be read from the call before)
  if (lane == 0) {
    shs[w] = s;
    shn[w] = n;
  }
  __syncthreads();
  s = shs[0];
  n = shn[0];
  for (int k = 1; k < WL_GT / 64; ++k) {
    s = __fadd_rn(s, shs[k]);
    n += shn[k];
  }
}

__device__ __forceinline__ float wl_block_z(const float* __restrict__ h, int j, bool one, float div) {
  const float s = one ? h[0] : __fadd_rn(__fadd_rn(__fadd_rn(h[j], h[j + 1]), h[j + 2]), h[j + 3]);
  return __fdiv_rn(s, div);
}

__device__ __forceinline__ float wl_lufs(float z) {   // -0.691 + 10 log10 z in fp64, rounded once; -inf for z == 0
  return z > 0.f ? (float)(-0.691 + 10.0 * log10((double)z)) : -INFINITY;
}

__global__ __launch_bounds__(WL_GT) void wl_gates_kernel(const float* __restrict__ h_all, int nhmax, const float* __restrict__ cmax_all,
                                                         int nch, const int32_t* __restrict__ samples, int H, float z_abs, int level,
                                                         float target, float ceiling, float* __restrict__ loud,
                                                         int32_t* __restrict__ blocks, int L) {
  __shared__ float shs[WL_GT / 64];
  __shared__ int shn[WL_GT / 64];
  const int b = blockIdx.x;
  const int n = wl_len(samples, b, L);
  const int nh = n / H;
  const bool one = nh < 4;
  const int nb = n == 0 ? 0 : (one ? 1 : nh - 3);
  const float div = one ? (float)n : (float)(4 * H);
  const float* h = h_all + (int64_t)b * nhmax;
  // the absolute gate
  float sa = 0.f, zmax = 0.f;
  int ca = 0;
  for (int j = threadIdx.x; j < nb; j += WL_GT) {
    const float z = wl_block_z(h, j, one, div);
    zmax = fmaxf(zmax, z);
    if (z > z_abs) {
      sa = __fadd_rn(sa, z);
      ++ca;
    }
  }
  wl_block_sum(sa, ca, shs, shn);
  // the relative gate, 10 LU below the mean of what passed the absolute one
  const float thr = ca > 0 ? __fmul_rn(0.1f, __fdiv_rn(sa, (float)ca)) : 0.f;
  float sb = 0.f;
  int cb = 0;
  for (int j = threadIdx.x; j < nb; j += WL_GT) {
    const float z = wl_block_z(h, j, one, div);
    if (z > z_abs && z > thr) {
      sb = __fadd_rn(sb, z);
      ++cb;
    }
  }
  wl_block_sum(sb, cb, shs, shn);
  // max z (for M) and the peak: maxima are exact in any order
  zmax = wave_max(zmax);
  float pk = 0.f;
  for (int k = threadIdx.x; (int64_t)k * WL_CHUNK < n; k += WL_GT) pk = fmaxf(pk, cmax_all[(int64_t)b * nch + k]);
  pk = wave_max(pk);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    shs[threadIdx.x >> 6] = zmax;
    shn[threadIdx.x >> 6] = __float_as_int(pk);
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int k = 1; k < WL_GT / 64; ++k) {
    zmax = fmaxf(zmax, shs[k]);
    pk = fmaxf(pk, __int_as_float(shn[k]));
  }
  const float I = cb > 0 ? wl_lufs(__fdiv_rn(sb, (float)cb)) : -INFINITY;
  const float M = wl_lufs(zmax);
  float g = 1.f, pk_out = pk;
  int limited = 0;
  if (level && cb > 0 && I > -INFINITY && pk > 0.f) {
    g = (float)pow(10.0, ((double)target - (double)I) / 20.0);
    if (__fmul_rn(pk, g) > ceiling) {
      g = __fdiv_rn(ceiling, pk);
      limited = 1;
    }
    pk_out = __fmul_rn(pk, g);   // max |x g| = fl(max |x| g): rounding is monotone
  }
  *reinterpret_cast<float4*>(loud + 4 * (int64_t)b) = make_float4(I, M, g, pk_out);
  *reinterpret_cast<int4*>(blocks + 4 * (int64_t)b) = make_int4(nb, ca, cb, limited);
}

__device__ __forceinline__ void wl_store4(float* p, const float* v) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ void wl_store4(int16_t* p, const int16_t* v) { *reinterpret_cast<short4*>(p) = make_short4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ void wl_convert(float v, float& o) { o = v; }
__device__ __forceinline__ void wl_convert(float v, int16_t& o) {
  o = (int16_t)(int)truncf(__fmul_rn(fminf(fmaxf(v, -1.f), 1.f), 32767.0f));
}

// dst[b, j] = x[b, j] g_b (T = float) or its PCM16 (T = int16_t) for j < n_b, 0 behind.  A thread owns 4 consecutive outputs that
// start on a 16-byte / 8-byte boundary of the ROW'S ADDRESS; whole groups are one vector store, a row's two edge groups scalar ones.
// Every output is read (as x[b, j]) and written by the same thread: dst may be the wave itself
template <typename T>
__global__ __launch_bounds__(WL_ET) void wl_emit_kernel(const float* wave, const int32_t* __restrict__ samples,
                                                        const float* __restrict__ loud, T* dst, int tiles, int L) {
  const int b = blockIdx.x / tiles, t = blockIdx.x % tiles;
  const int n = wl_len(samples, b, L);
  const float g = loud[4 * (int64_t)b + 2];
  T* row = dst + (int64_t)b * L;
  const float* x = wave + (int64_t)b * L;
  const int a = (int)((reinterpret_cast<uintptr_t>(row) / sizeof(T)) & 3);
  const int64_t j0 = ((int64_t)t * WL_ET + threadIdx.x) * WL_EPER - a;
  if (j0 >= L) return;
  T q[WL_EPER];
#pragma unroll
  for (int k = 0; k < WL_EPER; ++k) {
    const int64_t j = j0 + k;
    float v = 0.f;
    if (j >= 0 && j < n) v = __fmul_rn(x[j], g);
    wl_convert(v, q[k]);
  }
  if (j0 >= 0 && j0 + WL_EPER <= L) {
    wl_store4(row + j0, q);
  } else {
#pragma unroll
    for (int k = 0; k < WL_EPER; ++k)
      if (j0 + k >= 0 && j0 + k < L) row[j0 + k] = q[k];
  }
}

// ---- host: the coefficients, the powers of M, the workspace --------------------------------------------------------------------
bool wl_sr_ok(int sr) { return sr >= 8000 && sr <= 48000 && sr % 10 == 0; }

void wl_coefficients(int sr, double coef[10]) {
  const double pi = 3.14159265358979323846;
  {
    const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
    const double K = tan(pi * f0 / sr), Vh = pow(10.0, G / 20.0), Vb = pow(Vh, 0.4996667741545416);
    const double a0 = 1.0 + K / Q + K * K;
    coef[0] = (Vh + Vb * K / Q + K * K) / a0;
    coef[1] = 2.0 * (K * K - Vh) / a0;
    coef[2] = (Vh - Vb * K / Q + K * K) / a0;
    coef[3] = 2.0 * (K * K - 1.0) / a0;
    coef[4] = (1.0 - K / Q + K * K) / a0;
  }
  {
    const double f0 = 38.13547087602444, Q = 0.5003270373238773;
    const double K = tan(pi * f0 / sr), d = 1.0 + K / Q + K * K;
    coef[5] = 1.0;
    coef[6] = -2.0;
    coef[7] = 1.0;
    coef[8] = 2.0 * (K * K - 1.0) / d;
    coef[9] = (1.0 - K / Q + K * K) / d;
  }
}

struct WlMat64 {
  double m[4][4];
};
WlMat64 wl_mul(const WlMat64& x, const WlMat64& y) {
  WlMat64 r;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      double s = 0.0;
      for (int k = 0; k < 4; ++k) s += x.m[i][k] * y.m[k][j];
      r.m[i][j] = s;
    }
  return r;
}
WlMat wl_blocks(const WlMat64& x) {
  WlMat r;
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j) {
      r.a[2 * i + j] = x.m[i][j];
      r.c[2 * i + j] = x.m[2 + i][j];
      r.d[2 * i + j] = x.m[2 + i][2 + j];
    }
  return r;
}

// The device's filter is the one of the fp32 coefficients, so M is built from THEM (in fp64): the state maps then are those of the
// recursion the threads run
WlParams wl_params(int sr, WlCarryParams& q) {
  double cf[10];
  wl_coefficients(sr, cf);
  WlParams p;
  p.f = {(float)cf[0], (float)cf[1], (float)cf[2], (float)cf[3], (float)cf[4], (float)cf[8], (float)cf[9]};
  p.d = {p.f.sb0, p.f.sb1, p.f.sb2, p.f.sa1, p.f.sa2, p.f.ha1, p.f.ha2};
  const double a1 = p.d.sa1, a2 = p.d.sa2, c1 = p.d.ha1, c2 = p.d.ha2;
  WlMat64 m = {{{-a1, 1.0, 0.0, 0.0}, {-a2, 0.0, 0.0, 0.0}, {-2.0 - c1, 0.0, -c1, 1.0}, {1.0 - c2, 0.0, -c2, 0.0}}};
  for (int k = 0; k < 3; ++k) m = wl_mul(m, m);   // M^8
  p.run = wl_blocks(m);
  for (int k = 0; k < 6; ++k) {
    p.lane[k] = wl_blocks(m);   // M^(8 2^k)
    m = wl_mul(m, m);
  }
  p.wave = wl_blocks(m);   // M^512
  m = wl_mul(m, m);
  m = wl_mul(m, m);
  for (int k = 0; k < 6; ++k) {
    q.lane[k] = wl_blocks(m);   // M^(2048 2^k); the high ones underflow towards 0, which is what they are
    m = wl_mul(m, m);
  }
  return p;
}

int64_t wl_pitch(int L) { return ((int64_t)L + 3) & ~(int64_t)3; }
int wl_chunks(int L) { return cdiv(L, WL_CHUNK); }
int wl_hops(int L, int sr) { return std::max(1, L / (sr / 10)); }

// workspace of taco_wave_loudness: y (B, L rounded up to 4), the chunks' end states and carries (4 doubles each), the chunk maxima,
// the hop sums.  Every offset is a multiple of 4 floats up to cmax: y and agg are read by 16 bytes.
struct WlWs {
  float* y;
  double *agg, *carry;
  float *cmax, *h;
  int64_t bytes;
};
WlWs wl_ws(void* ws, int B, int L, int sr) {
  WsCarver c(ws);
  WlWs w;
  const int64_t nch = wl_chunks(L);
  w.y = c.take<float>(B * wl_pitch(L));
  w.agg = c.take<double>(B * nch * 4);
  w.carry = c.take<double>(B * nch * 4);
  w.cmax = c.take<float>(B * nch);
  w.h = c.take<float>((int64_t)B * wl_hops(L, sr));
  c.take<float>(64);   // slack, for nothing: a base that is not 16-byte aligned is refused.  Callers size buffers with it.
  w.bytes = c.bytes;
  return w;
}

}  // namespace

extern "C" int taco_k_weighting(int sr, double coef[10]) {
  TACO_REQUIRE(coef, "k_weighting: coef is NULL");
  TACO_REQUIRE(wl_sr_ok(sr), "k_weighting: sr=%d must be a multiple of 10 in [8000, 48000]", sr);
  wl_coefficients(sr, coef);
  return TACO_OK;
}

extern "C" int64_t taco_wave_loudness_workspace_bytes(int B, int L, int sr) {
  if (B <= 0 || L <= 0 || !wl_sr_ok(sr)) return TACO_EINVAL;
  return wl_ws(nullptr, B, L, sr).bytes;
}

extern "C" int taco_wave_loudness(const float* wave, const int32_t* samples, int sr, float target_lufs, float ceiling, float* out,
                                  int16_t* pcm, float* loud, int32_t* blocks, void* workspace, int B, int L, void* stream) {
  TACO_REQUIRE(wave && loud && blocks && workspace, "wave_loudness: wave, loud, blocks or workspace is NULL");
  TACO_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "wave_loudness: workspace is not 16-byte aligned");
  TACO_REQUIRE(B > 0 && L > 0, "wave_loudness: B=%d L=%d must be positive", B, L);
  TACO_REQUIRE(wl_sr_ok(sr), "wave_loudness: sr=%d must be a multiple of 10 in [8000, 48000]", sr);
  const int level = out || pcm;
  if (level) {
    TACO_REQUIRE(target_lufs >= -70.f && target_lufs <= 0.f, "wave_loudness: target_lufs %g is not in [-70, 0]", (double)target_lufs);   // (NaN fails)
    TACO_REQUIRE(ceiling > 0.f && ceiling <= 1.f, "wave_loudness: ceiling %g is not in (0, 1]", (double)ceiling);
  }
  const int nch = wl_chunks(L), nhmax = wl_hops(L, sr), H = sr / 10;
  const int tiles = cdiv((int64_t)L + 3, WL_ET * WL_EPER);   // groups of a row at its worst alignment
  TACO_REQUIRE((int64_t)B * tiles <= 0x7fffffff && B <= 65535, "wave_loudness: B=%d rows of L=%d are more than one grid holds", B, L);
  const int64_t pitch = wl_pitch(L);
  hipStream_t s = as_stream(stream);
  WlCarryParams q;
  const WlParams p = wl_params(sr, q);
  const float z_abs = (float)pow(10.0, (-70.0 + 0.691) / 10.0);
  const WlWs w = wl_ws(workspace, B, L, sr);
  float *y = w.y, *cmax = w.cmax, *h = w.h;
  double *agg = w.agg, *carry = w.carry;
  if (nch > 1) {
    TACO_KLAUNCH((wl_filter_kernel<true>), dim3(nch - 1, B), dim3(WL_T), 0, s, wave, samples, p, y, pitch, agg, nch, cmax, L);
    TACO_KLAUNCH(wl_carry_kernel, dim3(B), dim3(64), 0, s, agg, carry, samples, q, nch, L);
  }
  TACO_KLAUNCH((wl_filter_kernel<false>), dim3(nch, B), dim3(WL_T), 0, s, wave, samples, p, y, pitch, carry, nch, cmax, L);
  TACO_KLAUNCH(wl_hops_kernel, dim3(cdiv(nhmax, WL_NW), B), dim3(WL_T), 0, s, y, pitch, samples, h, nhmax, H, L);
  TACO_KLAUNCH(wl_gates_kernel, dim3(B), dim3(WL_GT), 0, s, h, nhmax, cmax, nch, samples, H, z_abs, level, target_lufs, ceiling, loud,
               blocks, L);
  if (pcm)   // (before out, which may overwrite the wave)
    TACO_KLAUNCH((wl_emit_kernel<int16_t>), dim3((unsigned)((int64_t)B * tiles)), dim3(WL_ET), 0, s, wave, samples, loud, pcm, tiles, L);
  if (out)
    TACO_KLAUNCH((wl_emit_kernel<float>), dim3((unsigned)((int64_t)B * tiles)), dim3(WL_ET), 0, s, wave, samples, loud, out, tiles, L);
  TACO_LAUNCH_CHECK("wave_loudness");
  return TACO_OK;
}
