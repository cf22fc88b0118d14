// limiter.hip -- true-peak meter and look-ahead limiter of finished waveforms (include/taco_hip.h taco_wave_limit).  No counterpart
// in the reference.  taco_wave_loudness honours its ceiling by holding the whole row's gain down; this stage takes the gain the
// target asks for and pulls down only the neighbourhood of a peak, and it puts the ceiling on the TRUE peak: the largest of the
// samples and of P - 1 interpolated phases between them (a polyphase FIR of T taps per phase).
//
// No recursion anywhere: an interpolating FIR, a sliding minimum, a smoothing FIR.  Every value is a single rounded fp32 operation
// in a stated order (no contraction), so the result is the same bits as the NumPy float32 restatement tests/limiter_ref.py.
//
// A row is cut into chunks of LM_CHUNK = 2048 samples at FIXED positions, one workgroup per chunk:
//   lm_halo     only when out is the wave itself: the H = 2 W + T / 2 samples on either side of every chunk, copied into the
//               workspace, so that no workgroup reads what its neighbour overwrites
//   lm_chunk<E> the chunk and its halo into LDS (x is read from memory once); the envelope e and the required gain r over
//               [-2 W, 2048 + 2 W), a thread owning 8 consecutive samples (lm_fir8); the sliding minimum m over [-W, 2048 + W) by
//               doubling in LDS; d, s and out for the chunk's own samples, 8 consecutive ones per thread again; out / pcm by
//               16-byte / 8-byte stores at any row alignment (wl_emit's form, per chunk); the chunk's max e, min s, max |out| and
//               count of s < 1 into the workspace.  E = false: the meter alone (e and max |x|)
//   lm_rows     one wave per row: the chunks' partials -> peaks, counts
// Two launches (three when out is the wave).  No workgroup waits for another one; maxima, minima and integer counts are exact in
// any order, and the two sums have the order of the contract.
// LDS: (2048 + 2 H) + (2048 + 4 W) floats and one of padding per 8, 37.1 KB at W = 512, T = 32; 19.6 KB at W = 24, T = 12.
#include <math.h>

#include "kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int LM_T = 256, LM_CHUNK = 2048, LM_PER = LM_CHUNK / LM_T, LM_NW = LM_T / 64;
constexpr int LM_PMAX = 8, LM_TMAX = 32, LM_WMAX = 512;
constexpr int LM_HPITCH_PAD = LM_TMAX / 2;                       // a halo in the workspace is 2 W + 16 floats, whatever T is
constexpr int LM_RPER = (LM_CHUNK + 4 * LM_WMAX) / LM_T;         // r values per thread at the largest W
static_assert(LM_CHUNK == TACO_LIMIT_CHUNK, "include/taco_hip.h states the chunk length");

// One rounded fp32 operation each.  Plain operators, compiled HERE under `fp contract(off)`: the header's __fmul_rn / __fadd_rn are
// `x * y` / `x + y` compiled under the header's default, and the pair fuses into one multiply-add once both are inlined -- a first
// build differed from the restatement by one unit in the last place for that reason
__device__ __forceinline__ float lm_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float lm_add(float a, float b) { return a + b; }
__device__ __forceinline__ float lm_sub(float a, float b) { return a - b; }
__device__ __forceinline__ float lm_div(float a, float b) { return a / b; }   // (IEEE: hipcc's default for fp32 division)

// LDS arrays are padded by one float per 8: a thread that owns 8 consecutive elements then is 9 floats from its neighbour, and the
// 64 lanes of a wave reading "my element + c" meet 64 different banks
__host__ __device__ __forceinline__ int lm_pad(int i) { return i + (i >> 3); }
__host__ __device__ __forceinline__ int lm_lds_floats(int n) { return lm_pad(n + LM_PER) + 1; }   // n elements and 8 behind them

// acc[q] = sum_{j < nt} fl(c[j] a[i0 + q + j]) for q = 0 .. 7, each accumulated from 0 in order of j, from the padded LDS array a.
// The 8 inputs of the current tap sit in registers: one LDS read per tap serves 8 products, and the register that element 0 is done
// with takes element 7's next input (the names rotate over 8 unrolled taps; the last taps' reads go up to 8 floats past what is
// used, which lm_lds_floats allocates).  c is uniform: 8 coefficients per scalar load, none inside the products
__device__ __forceinline__ void lm_fir8(const float* __restrict__ c, int nt, const float* a, int i0, float (&acc)[LM_PER]) {
  float v[LM_PER];
#pragma unroll
  for (int q = 0; q < LM_PER; ++q) {
    acc[q] = 0.f;
    v[q] = a[lm_pad(i0 + q)];
  }
  int j0 = 0;
  for (; j0 + LM_PER <= nt; j0 += LM_PER) {
    float t[LM_PER];
#pragma unroll
    for (int jj = 0; jj < LM_PER; ++jj) t[jj] = c[j0 + jj];
#pragma unroll
    for (int jj = 0; jj < LM_PER; ++jj) {
#pragma unroll
      for (int q = 0; q < LM_PER; ++q) acc[q] = lm_add(acc[q], lm_mul(t[jj], v[(q + jj) & (LM_PER - 1)]));
      v[jj] = a[lm_pad(i0 + j0 + jj + LM_PER)];
    }
  }
  float t[LM_PER - 1];
#pragma unroll
  for (int jj = 0; jj < LM_PER - 1; ++jj) t[jj] = c[j0 + jj < nt ? j0 + jj : nt - 1];
#pragma unroll
  for (int jj = 0; jj < LM_PER - 1; ++jj) {
    if (j0 + jj < nt) {   // (uniform)
#pragma unroll
      for (int q = 0; q < LM_PER; ++q) acc[q] = lm_add(acc[q], lm_mul(t[jj], v[(q + jj) & (LM_PER - 1)]));
      v[jj] = a[lm_pad(i0 + j0 + jj + LM_PER)];
    }
  }
}

__device__ __forceinline__ int lm_len(const int32_t* __restrict__ samples, int b, int L) {
  if (!samples) return L;
  const int n = samples[b];
  return n < 0 ? 0 : (n > L ? L : n);
}

__device__ __forceinline__ float lm_gain(const float* __restrict__ gain, int b) {
  if (!gain) return 1.f;
  const float g = gain[b];
  return g > 0.f && g < INFINITY ? g : 1.f;   // (NaN fails both)
}

__device__ __forceinline__ float lm_wave_min(float v) { return -wave_max(-v); }
__device__ __forceinline__ int lm_wave_add(int n) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
  return n;
}

__device__ __forceinline__ void lm_store4(float* p, const float* v) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ void lm_store4(int16_t* p, const int16_t* v) { *reinterpret_cast<short4*>(p) = make_short4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ void lm_convert(float v, float& o) { o = v; }
__device__ __forceinline__ void lm_convert(float v, int16_t& o) {   // taco_wave_loudness's rule
  o = (int16_t)(int)truncf(lm_mul(fminf(fmaxf(v, -1.f), 1.f), 32767.0f));
}

// row[base .. end) = os[0 .. end - base) (os == nullptr: zeros), as T.  A thread owns 4 consecutive outputs that start on a 16-byte /
// 8-byte boundary of the ADDRESS; whole groups inside [base, end) are one vector store, the chunk's two edge groups scalar ones
template <typename T>
__device__ __forceinline__ void lm_emit(T* row, const float* os, int64_t base, int64_t end) {
  const int a = (int)((reinterpret_cast<uintptr_t>(row + base) / sizeof(T)) & 3);
  for (int u = threadIdx.x; u < LM_CHUNK / 4 + 1; u += LM_T) {
    const int64_t j0 = base - a + 4 * (int64_t)u;
    if (j0 >= end) break;
    T q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t j = j0 + k;
      float v = 0.f;
      if (os && j >= base && j < end) v = os[j - base];
      lm_convert(v, q[k]);
    }
    if (j0 >= base && j0 + 4 <= end) {
      lm_store4(row + j0, q);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (j0 + k >= base && j0 + k < end) row[j0 + k] = q[k];
    }
  }
}

// halo[b, c, side, i] = x[base - H + i] (side 0) / x[base + 2048 + i] (side 1), i < H, 0 outside [0, n_b)
__global__ __launch_bounds__(LM_T) void lm_halo_kernel(const float* __restrict__ wave, const int32_t* __restrict__ samples,
                                                       float* __restrict__ halo, int hpitch, int H, int nch, int L) {
  const int c = blockIdx.x, b = blockIdx.y;
  const int n = lm_len(samples, b, L);
  const int64_t base = (int64_t)c * LM_CHUNK;
  if (base >= n) return;   // (nobody reads the halo of a chunk behind the row's end)
  const float* x = wave + (int64_t)b * L;
  float* h = halo + ((int64_t)b * nch + c) * 2 * hpitch;
  for (int i = threadIdx.x; i < 2 * H; i += LM_T) {
    const int side = i >= H, k = side ? i - H : i;
    const int64_t j = side ? base + LM_CHUNK + k : base - H + k;
    h[(int64_t)side * hpitch + k] = j >= 0 && j < n ? x[j] : 0.f;
  }
}

// part[b, c] = (max e, min s, max |out|, count of s < 1 as bits) of the chunk's samples inside [0, n_b); EMIT = false: (max e, 1,
// max |x|, 0).  wave and out are not restrict: out may be the wave (then halo is lm_halo_kernel's copy, else nullptr)
template <bool EMIT>
__global__ __launch_bounds__(LM_T) void lm_chunk_kernel(const float* wave, const int32_t* __restrict__ samples,
                                                        const float* __restrict__ gain, float ceiling, const float* __restrict__ taps,
                                                        int P, int T, const float* __restrict__ window, int W,
                                                        const float* __restrict__ halo, int hpitch, float* out, int16_t* pcm,
                                                        float* __restrict__ part, int nch, int L) {
  extern __shared__ float lm_sh[];
  __shared__ float red[3][LM_NW];
  __shared__ int redn[LM_NW];
  const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int n = lm_len(samples, b, L);
  const int64_t base = (int64_t)c * LM_CHUNK;
  const int64_t end = base + LM_CHUNK < L ? base + LM_CHUNK : L;
  if (base >= n) {   // (the whole workgroup) behind the row's end: zeros, and no partial that anybody reads
    if (EMIT) {
      if (pcm) lm_emit(pcm + (int64_t)b * L, nullptr, base, end);
      if (out) lm_emit(out + (int64_t)b * L, nullptr, base, end);
    }
    return;
  }
  const int half = T / 2, H = 2 * W + half;
  const int NX = LM_CHUNK + 2 * H, NR = LM_CHUNK + 4 * W;
  float* xs = lm_sh;                       // xs[lm_pad(i)] = x[base - H + i]
  float* rs = lm_sh + lm_lds_floats(NX);   // rs[lm_pad(i)] = r[base - 2 W + i], then the minima as 1 - m; at last the outputs, unpadded
  const float* x = wave + (int64_t)b * L;
  for (int i = tid; i < NX + LM_PER; i += LM_T) {
    const int64_t j = base - H + i;
    float v = 0.f;   // (also the LM_PER floats behind the array, which a thread's last group of a pass may read and never uses)
    if (i >= H && i < H + LM_CHUNK) {
      if (j < n) v = x[j];   // (samples from n_b on are never read)
    } else if (i >= NX) {
    } else if (halo) {
      const int side = i >= H;
      v = halo[(((int64_t)b * nch + c) * 2 + side) * hpitch + (side ? i - H - LM_CHUNK : i)];
    } else if (j >= 0 && j < n) {
      v = x[j];
    }
    xs[lm_pad(i)] = v;
  }
  __syncthreads();
  const float G = EMIT ? lm_gain(gain, b) : 1.f;
  // 1, 2: the envelope and the required gain.  Element i is sample base - 2 W + i = xs[i + T / 2]; tap j of it is xs[i + 1 + j].  A
  // thread owns LM_PER = 8 consecutive elements (lm_fir8)
  float emax = 0.f, xmax = 0.f;
  for (int i0 = LM_PER * tid; i0 < NR; i0 += LM_PER * LM_T) {
    float ax[LM_PER], e[LM_PER];
#pragma unroll
    for (int q = 0; q < LM_PER; ++q) e[q] = ax[q] = fabsf(xs[lm_pad(i0 + q + half)]);
    for (int p = 1; p < P; ++p) {
      const float* tp = taps + (p - 1) * T;
      float acc[LM_PER];
      lm_fir8(tp, T, xs, i0 + 1, acc);
#pragma unroll
      for (int q = 0; q < LM_PER; ++q) e[q] = fmaxf(e[q], fabsf(acc[q]));
    }
#pragma unroll
    for (int q = 0; q < LM_PER; ++q) {
      const int i = i0 + q;
      const int64_t j = base - 2 * W + i;
      const bool in = j >= 0 && j < n;
      if (in && i >= 2 * W && i < 2 * W + LM_CHUNK) {
        emax = fmaxf(emax, e[q]);
        xmax = fmaxf(xmax, ax[q]);
      }
      if (EMIT && i < NR) {
        float r = 1.f;
        if (in) {
          const float ge = lm_mul(G, e[q]);
          if (ge > ceiling) r = lm_div(ceiling, ge);
        }
        rs[lm_pad(i)] = r;
      }
    }
  }
  float smin = 1.f, omax = xmax;
  int cnt = 0;
  if (EMIT) {
    __syncthreads();
    const int t0 = LM_PER * tid;   // the thread's own samples of the chunk: t0 .. t0 + 7
    float rown[LM_PER];
#pragma unroll
    for (int q = 0; q < LM_PER; ++q) rown[q] = rs[lm_pad(2 * W + t0 + q)];
    // 3: m[i] = min rs[i .. i + 2 W] by doubling: after a pass of width `span`, rs[i] is the minimum over [i, i + 2 span) of what
    // the array holds; the last pass joins two such windows that cover 2 W + 1 and leaves 1 - m, the term of the sum below.  Every
    // pass reads, waits, writes, waits
    const int w = 2 * W + 1;
    int span = 1;
    for (;;) {
      const bool last = 2 * span > w;
      const int off = last ? w - span : span;
      float tmp[LM_RPER];
#pragma unroll
      for (int q = 0; q < LM_RPER; ++q) {
        const int i = tid + LM_T * q;
        if (i < NR) {
          float a = rs[lm_pad(i)];
          if (i + off < NR) a = fminf(a, rs[lm_pad(i + off)]);
          tmp[q] = last ? lm_sub(1.f, a) : a;
        }
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < LM_RPER; ++q) {
        const int i = tid + LM_T * q;
        if (i < NR) rs[lm_pad(i)] = tmp[q];
      }
      __syncthreads();
      if (last) break;
      span *= 2;
    }
    // 4, 5: sample t of the chunk sees m[t - W + k] = rs[t + k]
    float d[LM_PER];
    lm_fir8(window, w, rs, t0, d);
    float o[LM_PER];
#pragma unroll
    for (int q = 0; q < LM_PER; ++q) {
      const float s = fminf(lm_sub(1.f, d[q]), rown[q]);
      o[q] = 0.f;
      if (base + t0 + q < n) {
        o[q] = lm_mul(lm_mul(G, xs[lm_pad(H + t0 + q)]), s);
        smin = fminf(smin, s);
        cnt += s < 1.f;
      }
    }
    __syncthreads();   // (every read of the minima is done)
    omax = 0.f;
#pragma unroll
    for (int q = 0; q < LM_PER; ++q) {
      rs[t0 + q] = o[q];
      omax = fmaxf(omax, fabsf(o[q]));
    }
    __syncthreads();
    if (pcm) lm_emit(pcm + (int64_t)b * L, rs, base, end);
    if (out) lm_emit(out + (int64_t)b * L, rs, base, end);
  }
  const int lane = tid & 63, wv = tid >> 6;
  emax = wave_max(emax);
  smin = lm_wave_min(smin);
  omax = wave_max(omax);
  cnt = lm_wave_add(cnt);
  if (lane == 0) {
    red[0][wv] = emax;
    red[1][wv] = smin;
    red[2][wv] = omax;
    redn[wv] = cnt;
  }
  __syncthreads();
  if (tid != 0) return;
  for (int k = 1; k < LM_NW; ++k) {
    emax = fmaxf(emax, red[0][k]);
    smin = fminf(smin, red[1][k]);
    omax = fmaxf(omax, red[2][k]);
    cnt += redn[k];
  }
  float* pt = part + ((int64_t)b * nch + c) * 4;
  pt[0] = emax;
  pt[1] = smin;
  pt[2] = omax;
  pt[3] = __int_as_float(cnt);
}

template <bool EMIT>
__global__ __launch_bounds__(64) void lm_rows_kernel(const float* __restrict__ part, int nch, const int32_t* __restrict__ samples,
                                                     const float* __restrict__ gain, float* __restrict__ peaks,
                                                     int32_t* __restrict__ counts, int L) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int n = lm_len(samples, b, L);
  const int nc = (int)(((int64_t)n + LM_CHUNK - 1) / LM_CHUNK);
  float emax = 0.f, smin = 1.f, omax = 0.f;
  int cnt = 0;
  for (int c = lane; c < nc; c += 64) {
    const float* pt = part + ((int64_t)b * nch + c) * 4;
    emax = fmaxf(emax, pt[0]);
    smin = fminf(smin, pt[1]);
    omax = fmaxf(omax, pt[2]);
    cnt += __float_as_int(pt[3]);
  }
  emax = wave_max(emax);
  smin = lm_wave_min(smin);
  omax = wave_max(omax);
  cnt = lm_wave_add(cnt);
  if (lane != 0) return;
  peaks[4 * (int64_t)b + 0] = emax;
  peaks[4 * (int64_t)b + 1] = EMIT ? lm_gain(gain, b) : 1.f;
  peaks[4 * (int64_t)b + 2] = smin;
  peaks[4 * (int64_t)b + 3] = omax;
  counts[2 * (int64_t)b + 0] = n;
  counts[2 * (int64_t)b + 1] = cnt;
}

int lm_chunks(int L) { return cdiv(L, LM_CHUNK); }
bool lm_w_ok(int W) { return W >= 0 && W <= LM_WMAX; }

// workspace of taco_wave_limit: per chunk the four partials and (used only when out is the wave) its two halos of 2 W + 16 floats
struct LmWs {
  float *part, *halo;
  int64_t bytes;
};
LmWs lm_ws(void* ws, int B, int L, int W) {
  WsCarver c(ws);
  LmWs w;
  const int64_t chunks = (int64_t)B * lm_chunks(L);
  w.part = c.take<float>(chunks * 4);
  w.halo = c.take<float>(chunks * 2 * (2 * (int64_t)W + LM_HPITCH_PAD));
  c.take<float>(64);   // slack, for nothing: no array is aligned beyond the base.  Callers size buffers with it.
  w.bytes = c.bytes;
  return w;
}

}  // namespace

extern "C" int64_t taco_wave_limit_workspace_bytes(int B, int L, int W) {
  if (B <= 0 || L <= 0 || !lm_w_ok(W)) return TACO_EINVAL;
  return lm_ws(nullptr, B, L, W).bytes;
}

extern "C" int taco_wave_limit(const float* wave, const int32_t* samples, const float* gain, float ceiling, const float* taps, int P,
                               int T, const float* window, int W, float* out, int16_t* pcm, float* peaks, int32_t* counts,
                               void* workspace, int B, int L, void* stream) {
  TACO_REQUIRE(wave && peaks && counts && workspace, "wave_limit: wave, peaks, counts or workspace is NULL");
  TACO_REQUIRE(B > 0 && L > 0, "wave_limit: B=%d L=%d must be positive", B, L);
  TACO_REQUIRE(P >= 1 && P <= LM_PMAX, "wave_limit: P=%d is not in [1, %d]", P, LM_PMAX);
  TACO_REQUIRE(T >= 2 && T <= LM_TMAX && T % 2 == 0, "wave_limit: T=%d is not an even number in [2, %d]", T, LM_TMAX);
  TACO_REQUIRE(taps || P == 1, "wave_limit: taps is NULL with P=%d", P);
  const bool emit = out || pcm;
  if (emit) {
    TACO_REQUIRE(lm_w_ok(W), "wave_limit: W=%d is not in [0, %d]", W, LM_WMAX);
    TACO_REQUIRE(window, "wave_limit: window is NULL");
    TACO_REQUIRE(ceiling > 0.f && ceiling <= 1.f, "wave_limit: ceiling %g is not in (0, 1]", (double)ceiling);   // (NaN fails)
  } else {
    W = 0;   // the meter looks at neither gain, ceiling, window nor W
  }
  TACO_REQUIRE(B <= 65535, "wave_limit: B=%d rows are more than one grid holds", B);
  const int nch = lm_chunks(L), half = T / 2, H = 2 * W + half, hpitch = 2 * W + LM_HPITCH_PAD;
  hipStream_t s = as_stream(stream);
  const LmWs w = lm_ws(workspace, B, L, W);
  float* part = w.part;
  float* halo = nullptr;
  if (emit && out == wave) {
    halo = w.halo;
    TACO_KLAUNCH(lm_halo_kernel, dim3(nch, B), dim3(LM_T), 0, s, wave, samples, halo, hpitch, H, nch, L);
  }
  const size_t lds = (size_t)(lm_lds_floats(LM_CHUNK + 2 * H) + (emit ? lm_lds_floats(LM_CHUNK + 4 * W) : 0)) * sizeof(float);
  if (emit) {
    TACO_KLAUNCH((lm_chunk_kernel<true>), dim3(nch, B), dim3(LM_T), lds, s, wave, samples, gain, ceiling, taps, P, T, window, W, halo,
                 hpitch, out, pcm, part, nch, L);
    TACO_KLAUNCH((lm_rows_kernel<true>), dim3(B), dim3(64), 0, s, part, nch, samples, gain, peaks, counts, L);
  } else {
    TACO_KLAUNCH((lm_chunk_kernel<false>), dim3(nch, B), dim3(LM_T), lds, s, wave, samples, gain, ceiling, taps, P, T, window, W, halo,
                 hpitch, out, pcm, part, nch, L);
    TACO_KLAUNCH((lm_rows_kernel<false>), dim3(B), dim3(64), 0, s, part, nch, samples, gain, peaks, counts, L);
  }
  TACO_LAUNCH_CHECK("wave_limit");
  return TACO_OK;
}
