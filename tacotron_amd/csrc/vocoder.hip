// vocoder.hip -- Griffin-Lim phase reconstruction on the GPU (audio.griffinlim / invert_spectrogram,
// audio.py:69-97: 50 rounds of librosa.istft -> librosa.stft with n_fft 2048, win_length 1200, hop_length 300, 'hann').
//
// One workgroup (256 threads) owns one frame: a 2048-point complex FFT in LDS (in-place radix-2, bit-reversed load, a
// 1024-entry twiddle table computed once per workgroup with sincospif), no vendor FFT.  One Griffin-Lim round is two launches:
//   gl_synth : frame t: Hermitian-extend mag * e^{i angle} -> inverse FFT -> times the zero-padded periodic Hann window ->
//              the 1200 non-zero samples of the frame's segment to `seg` (B, F, 1200)
//   gl_anal  : frame t: gather its 2048 input samples on the fly = overlap-add of <= 4 segments, divided by the window
//              sum-of-squares, trimmed by n_fft/2 and reflect-padded exactly as librosa's center=True STFT does -> window ->
//              forward FFT -> new unit-modulus angles (B, F, 1025)
// The overlap-add is a GATHER (each output sample sums the segments that cover it, in frame order): no atomics, results are
// reproducible.  gl_wave applies the same gather once more for the final waveform.
//
// Per-utterance frame counts (taco_griffinlim_rows): every kernel takes the row pitch F, a nullable device array `frames` and a
// multiplier; row b is vocoded over its first F_b = min(F, frames[b] * multiplier) frames (frames == nullptr: F_b = F, which is
// how taco_griffinlim launches the SAME kernels -- device code is compiled with floating-point contraction on, so only one body
// for both entry points makes a row of the rows form bit-identical to taco_griffinlim of that row alone).  F_b replaces F in the
// reflect padding, the overlap-add and the window normalisation; the addressing of mag_t, phases, segments and angles keeps the
// pitch F.  A frame workgroup with t >= F_b returns at entry, before it builds its twiddle table: the grid stays (F, B) because
// the host never learns the lengths, and the frames past a row's end cost one integer load and a compare.
//
// Fast Griffin-Lim (taco_griffinlim_fast; Perraudin, Balazs, Sondergaard 2013) and the convergence readout live in the epilogue of
// the SAME analysis body, as template parameters: MOM keeps the previous round's spectrum t_{i-1} in a second (B, F, 1025, 2)
// buffer and takes the phases of c_i = t_i + alpha (t_i - t_{i-1}); CONV reduces (|t_i[k]| - M[k])^2 over the frame's bins in a
// fixed order (wave butterfly, then the four wave sums in LDS) into a (B, F) scratch that gl_conv_kernel sums per row, again in
// an order that depends on F_b alone; WRITE = false is the readout's own last pass, which stores no angles.  The instantiation
// <false, false, true> is the body both older entry points launch; alpha = 0 launches it as well.
//
// Waveform finishing (taco_wave_finish) follows the Griffin-Lim kernels below: the de-emphasis scan, the energy trim, the peak and
// the fp32 / PCM16 emit of the waveform gl_wave_kernel wrote.  Joining the finished pieces of a long prompt (taco_wave_join) comes
// last: the pieces' offsets, the joined fp32 row with its edge ramps, the prompt's peak and PCM16.
#include <algorithm>

#include "kernels.h"
#include "stft.h"

namespace {

// in-place 2048-point FFT of (re, im) in LDS, plain index (stft.h fft_stages); the results are visible to every thread on return
__device__ __forceinline__ void fft2048(float* re, float* im, const float* twr, const float* twi, float sign) {
  fft_stages<11>(re, im, twr, twi, sign, LdsPlain());
  __syncthreads();
}

// sum of v over the 256 threads of the workgroup in a fixed order, returned to every thread: xor butterfly inside each wave, then
// the four wave sums through sh (4 floats of LDS nobody else touches until the next barrier) as (s0 + s1) + (s2 + s3).
// NOT elementwise.hip's block_sum: that one takes any block size and adds the wave sums in sequence -- other bits.
__device__ __forceinline__ float block_sum4(float v, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// frames of row b: F without a frames array, else min(F, frames[b] * per_unit); a row below 5 frames (the reflect padding of
// n_fft/2 needs more than 1024 samples) has none
__device__ __forceinline__ int row_frames(const int32_t* __restrict__ frames, int per_unit, int b, int F) {
  if (!frames) return F;
  const int64_t n = (int64_t)frames[b] * per_unit;
  if (n < 5) return 0;
  return n > F ? F : (int)n;
}

// window sum-of-squares (librosa.filters.window_sumsquare) of row blockIdx.y over n = NFFT + HOP (F_b - 1) samples; rows are
// `pitch` floats apart (0: one table for a batch whose rows all have F frames)
__global__ void gl_wss_kernel(float* __restrict__ wss_all, int64_t pitch, int Fp, const int32_t* __restrict__ frames, int per_unit) {
  const int F = row_frames(frames, per_unit, blockIdx.y, Fp);
  if (F == 0) return;
  float* wss = wss_all + (int64_t)blockIdx.y * pitch;
  const int n = NFFT + HOP * (F - 1);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    float acc = 0.f;
    // frames t with t*HOP + WOFF <= i < t*HOP + WOFF + WIN
    int t_hi = (i - WOFF) / HOP;
    if (i - WOFF < 0) t_hi = -1;
    for (int t = t_hi; t >= 0 && t > t_hi - 4; --t) {
      const int j = i - t * HOP - WOFF;
      if (t < F && j >= 0 && j < WIN) {
        const float w = hann(j);
        acc += w * w;
      }
    }
    wss[i] = acc;
  }
}

// angles (B, F, NBIN, 2) <- unit phasors of the given phase angles (radians), or, phase == nullptr, of the counter-hash phases
// of taco_griffinlim_rows: element (b, k, t) of the (B, NBIN, F) matrix has index j, u = splitmix64(seed * C + j) >> 40 (24 bits)
// and the angle 2 pi u / 2^24; 2 u / 2^24 is exact in fp32.  Frames t >= F_b are left alone.
__global__ void gl_init_kernel(const float* __restrict__ phase, uint64_t seed, float* __restrict__ ang, int F, int64_t total,
                               const int32_t* __restrict__ frames, int per_unit) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t bt = i / NBIN;
    const int k = (int)(i - bt * NBIN);
    const int64_t b = bt / F;
    const int t = (int)(bt - b * F);
    if (t >= row_frames(frames, per_unit, (int)b, F)) continue;
    const int64_t j = (b * NBIN + k) * F + t;   // phase is (B, NBIN, F) like the magnitude matrix
    float s, c;
    if (phase) {
      sincosf(phase[j], &s, &c);
    } else {
      const uint32_t u = (uint32_t)(counter_hash(seed, (uint64_t)j) >> 40);
      sincospif((float)u * (2.0f / 16777216.0f), &s, &c);
    }
    ang[i * 2] = c;
    ang[i * 2 + 1] = s;
  }
}

__global__ __launch_bounds__(FT) void gl_synth_kernel(const float* __restrict__ mag_t, const float* __restrict__ ang,
                                                      float* __restrict__ seg, int F,
                                                      const int32_t* __restrict__ frames, int per_unit) {
  __shared__ float re[NFFT], im[NFFT], twr[NFFT / 2], twi[NFFT / 2];
  const int t = blockIdx.x, b = blockIdx.y;
  if (t >= row_frames(frames, per_unit, b, F)) return;   // (the whole workgroup: nothing of this frame is ever read)
  make_twiddles(twr, twi);
  const float* a = ang + ((int64_t)b * F + t) * NBIN * 2;
  const float* m = mag_t + (int64_t)b * NBIN * F + t;
  // X[k] = mag e^{i angle}, Hermitian extension X[N - k] = conj(X[k]); stored bit-reversed for the in-place FFT
  for (int k = threadIdx.x; k < NBIN; k += FT) {
    const float mg = fabsf(m[(int64_t)k * F]);
    const float xr = mg * a[2 * k], xi = mg * a[2 * k + 1];
    const int r0 = bitrev<11>(k);
    re[r0] = xr; im[r0] = xi;
    if (k > 0 && k < NFFT / 2) {
      const int r1 = bitrev<11>(NFFT - k);
      re[r1] = xr; im[r1] = -xi;
    }
  }
  fft2048(re, im, twr, twi, +1.0f);
  float* o = seg + ((int64_t)b * F + t) * WIN;
  for (int j = threadIdx.x; j < WIN; j += FT) o[j] = re[WOFF + j] * (1.0f / NFFT) * hann(j);
}

// sample i of the overlap-added, normalised signal of length NFFT + HOP (F - 1) (before the centre trim); F = the row's frames
__device__ __forceinline__ float ola_sample(const float* __restrict__ seg_b, const float* __restrict__ wss, int i, int F) {
  float acc = 0.f;
  int t_hi = (i - WOFF) / HOP;
  if (i - WOFF < 0) return 0.f;
  if (t_hi > F - 1) t_hi = F - 1;
  // frames in increasing order (fixed summation order)
  int t_lo = t_hi - 3;
  if (t_lo < 0) t_lo = 0;
  for (int t = t_lo; t <= t_hi; ++t) {
    const int j = i - t * HOP - WOFF;
    if (j >= 0 && j < WIN) acc += seg_b[(int64_t)t * WIN + j];
  }
  const float w = wss[i];
  return w > 1.17549435e-38f ? acc / w : acc;
}

// momentum / readout arguments of gl_anal_kernel (unused ones are null / 0)
struct GlExtra {
  float* tprev;         // MOM: (B, F, NBIN, 2) spectrum of the previous round, interleaved like ang
  float alpha;          // MOM: momentum
  int read_prev;        // MOM: 0 in round 0 (the buffer holds nothing yet and is not read)
  int write_prev;       // MOM: 0 in the last round (nobody reads it)
  const float* mag_t;   // CONV: the magnitudes (B, NBIN, F)
  float* part;          // CONV: (B, F) sum over the frame's bins of (|t[k]| - M[k])^2
};

template <bool MOM, bool CONV, bool WRITE>
__global__ __launch_bounds__(FT) void gl_anal_kernel(const float* __restrict__ seg, const float* __restrict__ wss,
                                                     int64_t wss_pitch, float* __restrict__ ang, int Fp,
                                                     const int32_t* __restrict__ frames, int per_unit, GlExtra x) {
  __shared__ float re[NFFT], im[NFFT], twr[NFFT / 2], twi[NFFT / 2];
  const int t = blockIdx.x, b = blockIdx.y;
  const int F = row_frames(frames, per_unit, b, Fp);   // frames of this row; Fp = the pitch
  if (t >= F) return;
  make_twiddles(twr, twi);
  wss += (int64_t)b * wss_pitch;
  const int L = HOP * (F - 1);   // length of the trimmed signal y
  const float* sb = seg + (int64_t)b * Fp * WIN;
  for (int j = threadIdx.x; j < NFFT; j += FT) {
    float v = 0.f;
    if (j >= WOFF && j < WOFF + WIN) {
      // padded signal index p = t*HOP + j over yp = reflect_pad(y, NFFT/2): y index q = p - NFFT/2 reflected into [0, L)
      int q = t * HOP + j - NFFT / 2;
      if (q < 0) q = -q;
      if (q >= L) q = 2 * (L - 1) - q;
      v = ola_sample(sb, wss, q + NFFT / 2, F) * hann(j - WOFF);
    }
    const int r0 = bitrev<11>(j);
    re[r0] = v;
    im[r0] = 0.f;
  }
  fft2048(re, im, twr, twi, -1.0f);
  float* a = ang + ((int64_t)b * Fp + t) * NBIN * 2;
  float dev2 = 0.f;
  for (int k = threadIdx.x; k < NBIN; k += FT) {
    float xr = re[k], xi = im[k];
    if constexpr (CONV) {
      const float d = sqrtf(xr * xr + xi * xi) - fabsf(x.mag_t[((int64_t)b * NBIN + k) * Fp + t]);
      dev2 += d * d;
    }
    if constexpr (MOM) {   // c = t + alpha (t - t_prev); t takes t_prev's place
      float2* p = reinterpret_cast<float2*>(x.tprev + ((int64_t)b * Fp + t) * NBIN * 2) + k;
      const float tr = xr, ti = xi;
      if (x.read_prev) {
        const float2 pv = *p;
        xr = tr + x.alpha * (tr - pv.x);
        xi = ti + x.alpha * (ti - pv.y);
      }
      if (x.write_prev) *p = make_float2(tr, ti);
    }
    if constexpr (WRITE) {
      const float n2 = xr * xr + xi * xi;
      float c = 1.f, s = 0.f;   // np.angle(0) = 0
      if (n2 > 0.f) {
        const float inv = rsqrtf(n2);
        c = xr * inv;
        s = xi * inv;
      }
      a[2 * k] = c;
      a[2 * k + 1] = s;
    }
  }
  if constexpr (CONV) {   // (the twiddle table is dead after the FFT's last barrier: its first floats carry the wave sums)
    const float tot = block_sum4(dev2, twr);
    if (threadIdx.x == 0) x.part[(int64_t)b * Fp + t] = tot;
  }
}

// mpart (B, F) <- sum over the bins of M[k]^2 of frame t < F_b (once per call, for the readout's denominator)
__global__ __launch_bounds__(FT) void gl_magsq_kernel(const float* __restrict__ mag_t, float* __restrict__ mpart, int F,
                                                      const int32_t* __restrict__ frames, int per_unit) {
  __shared__ float sh[4];
  const int t = blockIdx.x, b = blockIdx.y;
  if (t >= row_frames(frames, per_unit, b, F)) return;
  const float* m = mag_t + (int64_t)b * NBIN * F + t;
  float acc = 0.f;
  for (int k = threadIdx.x; k < NBIN; k += FT) {
    const float v = m[(int64_t)k * F];
    acc += v * v;
  }
  const float tot = block_sum4(acc, sh);
  if (threadIdx.x == 0) mpart[(int64_t)b * F + t] = tot;
}

// conv[b, col] <- sqrt(sum_t part[b, t] / sum_t mpart[b, t]) over the row's F_b frames, 0 for a row without frames or magnitudes.
// Thread j sums the frames j, j + 256, ... and block_sum4 the threads: the order depends on F_b alone.  first: sum mpart into
// msq[b]; later rounds read it back.
__global__ __launch_bounds__(FT) void gl_conv_kernel(const float* __restrict__ part, const float* __restrict__ mpart,
                                                     float* __restrict__ msq, float* __restrict__ conv, int col, int ncol, int Fp,
                                                     const int32_t* __restrict__ frames, int per_unit, int first) {
  __shared__ float sh[8];
  const int b = blockIdx.x;
  const int F = row_frames(frames, per_unit, b, Fp);
  float acc = 0.f, macc = 0.f;
  for (int t = threadIdx.x; t < F; t += FT) {
    acc += part[(int64_t)b * Fp + t];
    if (first) macc += mpart[(int64_t)b * Fp + t];
  }
  const float num = block_sum4(acc, sh);
  float den;
  if (first) {
    den = block_sum4(macc, sh + 4);
    if (threadIdx.x == 0) msq[b] = den;
  } else {
    den = msq[b];
  }
  if (threadIdx.x == 0) conv[(int64_t)b * ncol + col] = (F > 0 && den > 0.f) ? sqrtf(num / den) : 0.f;
}

// every sample of the row: the overlap-add below HOP (F_b - 1), 0 from there on
__global__ void gl_wave_kernel(const float* __restrict__ seg, const float* __restrict__ wss, int64_t wss_pitch,
                               float* __restrict__ wave, int Fp, const int32_t* __restrict__ frames, int per_unit) {
  const int L = HOP * (Fp - 1);
  const int b = blockIdx.y;
  const int F = row_frames(frames, per_unit, b, Fp);
  const int Lb = F > 0 ? HOP * (F - 1) : 0;
  wss += (int64_t)b * wss_pitch;
  const float* sb = seg + (int64_t)b * Fp * WIN;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < L; i += gridDim.x * blockDim.x)
    wave[(int64_t)b * L + i] = i < Lb ? ola_sample(sb, wss, i + NFFT / 2, F) : 0.f;
}

// ---- waveform finishing (taco_hip.h taco_wave_finish): de-emphasis, energy trim, peak, fp32 / PCM16 emit ---------------------
// y[n] = x[n] + a y[n-1] is a first-order linear scan: sample n is the map c -> a c + x[n], and maps compose as
// (A, B) o (A', B') = (A A', B' + A' B).  A row is cut into chunks of WF_CHUNK samples at FIXED positions (chunk c = samples
// [2048 c, 2048 c + 2048) of the row, whatever B and L are), one workgroup per chunk:
//   wf_scan<true>   the chunk's end value from a zero carry, into the workspace (only chunks that have a successor)
//   wf_scan<false>  the carry into chunk c rebuilt from the aggregates 0 .. c-1 in order (c fused multiply-adds with a^2048, formed
//                   by eleven squarings -- nothing assumes that it underflows), the scan again, y and max |y| of every 512 samples
//                   (one wave's share) into the workspace
//   wf_ms           mean square of the trim frames of y (one wave per frame), only with a trim
//   wf_bounds       one workgroup per row: the bounds from the frame energies, the peak from the 512-sample maxima
//   wf_emit         out / pcm shifted by the row's start
// No workgroup waits for another one inside a launch; the order of every sum depends on the position in the row and n_b alone.
constexpr int WF_T = 256, WF_PER = 8, WF_CHUNK = WF_T * WF_PER;
constexpr int WF_BT = 512;   // wf_bounds block

__device__ __forceinline__ int wf_len(const int32_t* __restrict__ samples, int b, int L) {
  if (!samples) return L;
  const int n = samples[b];
  return n < 0 ? 0 : (n > L ? L : n);
}

template <bool AGG>
__global__ __launch_bounds__(WF_T) void wf_scan_kernel(const float* __restrict__ wave, const int32_t* __restrict__ samples, float a,
                                                       float* __restrict__ y_all, int64_t y_pitch, float* __restrict__ agg_all,
                                                       int nch, float* __restrict__ pm_all, int npm, int L) {
  __shared__ float shA[WF_T / 64], shB[WF_T / 64];
  const int c = blockIdx.x, b = blockIdx.y;
  const int n = wf_len(samples, b, L);
  const int64_t base = (int64_t)c * WF_CHUNK;
  if (AGG ? base + WF_CHUNK >= n : base >= n) return;   // (the whole workgroup) AGG: nobody reads the last chunk's aggregate
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const float* x = wave + (int64_t)b * L;
  const int64_t i0 = base + (int64_t)threadIdx.x * WF_PER;
  float v[WF_PER];
  if (i0 + WF_PER <= n && (reinterpret_cast<uintptr_t>(x + i0) & 15) == 0) {
    const float4 p = *reinterpret_cast<const float4*>(x + i0), q = *reinterpret_cast<const float4*>(x + i0 + 4);
    v[0] = p.x; v[1] = p.y; v[2] = p.z; v[3] = p.w;
    v[4] = q.x; v[5] = q.y; v[6] = q.z; v[7] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < WF_PER; ++j) v[j] = i0 + j < n ? x[i0 + j] : 0.f;   // (samples from n_b on are never read)
  }
  float y[WF_PER];
  if (a == 0.f) {   // y = x bit for bit (a fused multiply-add with 0 would turn -0 into +0)
#pragma unroll
    for (int j = 0; j < WF_PER; ++j) y[j] = v[j];
  } else {
    // the thread's own samples from a zero carry, and a^(j+1)
    float pw[WF_PER];
    y[0] = v[0];
    pw[0] = a;
#pragma unroll
    for (int j = 1; j < WF_PER; ++j) {
      y[j] = fmaf(a, y[j - 1], v[j]);
      pw[j] = __fmul_rn(pw[j - 1], a);
    }
    // inclusive scan of the threads' maps (A, Bv) over the wave: the later map's A multiplies the earlier map's end value
    float A = pw[WF_PER - 1], Bv = y[WF_PER - 1];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const float Ap = __shfl_up(A, d), Bp = __shfl_up(Bv, d);
      if (lane >= d) {
        Bv = fmaf(A, Bp, Bv);
        A = __fmul_rn(A, Ap);
      }
    }
    float Aex = __shfl_up(A, 1), Bex = __shfl_up(Bv, 1);
    if (lane == 0) {
      Aex = 1.f;
      Bex = 0.f;
    }
    if (lane == 63) {
      shA[w] = A;
      shB[w] = Bv;
    }
    __syncthreads();
    float carry = 0.f;   // y[base - 1]
    if (!AGG) {
      float a2k = a;
#pragma unroll
      for (int k = 0; k < 11; ++k) a2k = __fmul_rn(a2k, a2k);   // a^2048
      const float* agg = agg_all + (int64_t)b * nch;
      for (int k = 0; k < c; ++k) carry = fmaf(a2k, carry, agg[k]);
    }
    for (int k = 0; k < w; ++k) carry = fmaf(shA[k], carry, shB[k]);   // ... the end value of the wave in front
    const float E = fmaf(Aex, carry, Bex);                              // ... of the thread in front
#pragma unroll
    for (int j = 0; j < WF_PER; ++j) y[j] = fmaf(pw[j], E, y[j]);
  }
  if (AGG) {
    if (threadIdx.x == WF_T - 1) agg_all[(int64_t)b * nch + c] = y[WF_PER - 1];
    return;
  }
  float* yo = y_all + (int64_t)b * y_pitch + i0;   // (16-byte aligned: the pitch is a multiple of 4 floats, i0 of 8)
  float m = 0.f;
  if (i0 + WF_PER <= n) {
    *reinterpret_cast<float4*>(yo) = make_float4(y[0], y[1], y[2], y[3]);
    *reinterpret_cast<float4*>(yo + 4) = make_float4(y[4], y[5], y[6], y[7]);
#pragma unroll
    for (int j = 0; j < WF_PER; ++j) m = fmaxf(m, fabsf(y[j]));
  } else {
#pragma unroll
    for (int j = 0; j < WF_PER; ++j)
      if (i0 + j < n) {
        yo[j] = y[j];
        m = fmaxf(m, fabsf(y[j]));
      }
  }
  m = wave_max(m);   // the wave's 512 samples
  const int64_t blk = base / 512 + w;
  if (lane == 0 && blk * 512 < n) pm_all[(int64_t)b * npm + blk] = m;
}

// ms[b, t] = mean square of trim frame t of y (2048 samples at hop 512 of the row reflect-padded by 1024); one wave per frame
__global__ __launch_bounds__(WF_T) void wf_ms_kernel(const float* __restrict__ y_all, int64_t y_pitch, const int32_t* __restrict__ samples,
                                                     float* __restrict__ ms_all, int nms, int L) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int n = wf_len(samples, b, L);
  const int t = blockIdx.x * (WF_T / 64) + (threadIdx.x >> 6);
  if (n == 0 || t >= 1 + n / TRIM_HOP) return;
  const float m = trim_frame_ms(y_all + (int64_t)b * y_pitch, n, t, lane);
  if (lane == 0) ms_all[(int64_t)b * nms + t] = m;
}

// one workgroup per row: bounds (stft.h's trim rule; top_db == 0: no trim) and the peak
__global__ __launch_bounds__(WF_BT) void wf_bounds_kernel(const float* __restrict__ ms_all, int nms, const float* __restrict__ pm_all,
                                                          int npm, const int32_t* __restrict__ samples, float top_db,
                                                          int32_t* __restrict__ bounds, float* __restrict__ peak, int L) {
  constexpr int NW = WF_BT / 64;
  __shared__ float red_max[NW];
  __shared__ int red_lo[NW], red_hi[NW];
  const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int n = wf_len(samples, b, L);
  int start = 0, end = n;
  if (top_db > 0.f && n > 0) {   // (uniform)
    const float* ms = ms_all + (int64_t)b * nms;
    const int nt = 1 + n / TRIM_HOP;
    float mx = 0.f;
    for (int t = threadIdx.x; t < nt; t += WF_BT) mx = fmaxf(mx, ms[t]);
    mx = wave_max(mx);
    if (lane == 0) red_max[w] = mx;
    __syncthreads();
    mx = red_max[0];
    for (int i = 1; i < NW; ++i) mx = fmaxf(mx, red_max[i]);
    const float ref_db = trim_db(mx);
    int lo = 0x7fffffff, hi = -1;
    for (int t = threadIdx.x; t < nt; t += WF_BT)
      if (trim_pass(ms[t], ref_db, top_db)) {
        lo = min(lo, t);
        hi = max(hi, t);
      }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo = min(lo, __shfl_xor(lo, o));
      hi = max(hi, __shfl_xor(hi, o));
    }
    if (lane == 0) {
      red_lo[w] = lo;
      red_hi[w] = hi;
    }
    __syncthreads();
    for (int i = 0; i < NW; ++i) {
      lo = min(lo, red_lo[i]);
      hi = max(hi, red_hi[i]);
    }
    trim_bounds(lo, hi, n, start, end);
    __syncthreads();   // red_max is used again below
  }
  // start is a multiple of 512 and end is one or n: the 512-sample maxima tile [start, end) exactly
  const float* pm = pm_all + (int64_t)b * npm;
  float pk = 0.f;
  for (int k = start / 512 + threadIdx.x; (int64_t)k * 512 < end; k += WF_BT) pk = fmaxf(pk, pm[k]);
  pk = wave_max(pk);
  if (lane == 0) red_max[w] = pk;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < NW; ++i) pk = fmaxf(pk, red_max[i]);
    bounds[2 * b] = start;
    bounds[2 * b + 1] = end;
    peak[b] = pk;
  }
}

// out[b, i] = y[s_b + i], pcm[b, i] = pcm16(y, peak) for i < e_b - s_b, zeros behind
__global__ __launch_bounds__(256) void wf_emit_kernel(const float* __restrict__ y_all, int64_t y_pitch, const int32_t* __restrict__ bounds,
                                                      const float* __restrict__ peak, float* __restrict__ out,
                                                      int16_t* __restrict__ pcm, int L) {
  const int b = blockIdx.y;
  const int s = bounds[2 * b], m = bounds[2 * b + 1] - s;
  const float pk = peak[b];
  const float* y = y_all + (int64_t)b * y_pitch + s;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < L; i += (int64_t)gridDim.x * 256) {
    const float v = i < m ? y[i] : 0.f;
    if (out) out[(int64_t)b * L + i] = v;
    if (pcm) pcm[(int64_t)b * L + i] = pcm16(v, pk);
  }
}

// ---- joining finished pieces (taco_hip.h taco_wave_join): offsets, joined fp32 rows with edge ramps, peak, PCM16 ---------------
//   wj_offsets  one workgroup per prompt: o_i = sum of len + gap of the pieces in front, an integer scan over chunks of 256 pieces
//               with a 64-bit carry (any number of pieces per prompt); offsets (clamped to Lj) and total
//   wj_emit     one workgroup per (prompt, tile of 1024 outputs): the piece under an output by binary search in the prompt's
//               offsets -- the clamped ones are enough: a piece at or behind Lj is under no output -- then the sample, ramped at
//               interior edges, or 0 in a gap; max |v| of the tile into the workspace
//   wj_pcm      one workgroup per (prompt, tile): the prompt's peak from its tile maxima (every workgroup forms it; the first one
//               of a prompt stores it), then PCM16 of the joined fp32 row
// A thread owns 4 consecutive outputs that start on a 16-byte (fp32) / 8-byte (int16) boundary of the ROW'S ADDRESS, whatever Lj and
// the pointer are: chunk c of a row that begins `a` elements behind such a boundary covers outputs [4c - a, 4c - a + 4); whole chunks
// are one vector store, the two edge chunks scalar ones.  The source is read by scalars (it is misaligned against the destination by
// offsets[i] % 4 in general; a wave still reads 1 KiB of consecutive floats).  Maxima are exact in any order and the scan is in
// integers: nothing depends on P, on the tiling or on the alignment.  No workgroup waits for another one.
constexpr int WJ_T = 256, WJ_PER = 4, WJ_TILE = WJ_T * WJ_PER;

__device__ __forceinline__ int wj_len(const int32_t* __restrict__ bounds, int i, int L) {
  const int64_t n = (int64_t)bounds[2 * i + 1] - (int64_t)bounds[2 * i];
  return n < 0 ? 0 : (n > L ? L : (int)n);
}

__global__ __launch_bounds__(WJ_T) void wj_offsets_kernel(const int32_t* __restrict__ bounds, const int32_t* __restrict__ first,
                                                          const int32_t* __restrict__ gap, int32_t* __restrict__ offsets,
                                                          int32_t* __restrict__ total, int L, int Lj) {
  __shared__ long long sh[WJ_T / 64];
  const int p = blockIdx.x, lo = first[p], hi = first[p + 1];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lo == hi) {   // (uniform) a prompt without pieces
    if (threadIdx.x == 0) total[p] = 0;
    return;
  }
  long long carry = 0;   // o of the chunk's first piece
  for (int64_t base = lo; base < hi; base += WJ_T) {   // (uniform)
    const int i = base + threadIdx.x < hi ? (int)(base + threadIdx.x) : -1;
    int len = 0;
    long long step = 0;
    if (i >= 0) {
      len = wj_len(bounds, i, L);
      step = (long long)len + (i + 1 < hi ? (long long)gap[i] : 0);   // (the gap behind a prompt's last piece is ignored)
    }
    long long inc = step;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const long long t = __shfl_up(inc, d);
      if (lane >= d) inc += t;
    }
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    long long o = carry + inc - step;
    for (int k = 0; k < w; ++k) o += sh[k];
    if (i >= 0) {
      offsets[i] = (int32_t)(o < Lj ? o : Lj);
      if (i == hi - 1) total[p] = (int32_t)(o + len < Lj ? o + len : Lj);
    }
    carry += (sh[0] + sh[1]) + (sh[2] + sh[3]);
    __syncthreads();   // sh is written again in the next chunk
  }
}

// sample n < len of piece i (row `src`), ramped when it lies within f = min(fade, len / 2) samples of an interior edge
__device__ __forceinline__ float wj_sample(const float* __restrict__ src, int n, int len, int fade, bool is_first, bool is_last) {
  const float x = src[n];
  const int f = min(fade, len >> 1);
  if (f > 0) {
    if (!is_first && n < f) return __fmul_rn(x, __fdiv_rn(__fadd_rn((float)n, 0.5f), (float)f));
    if (!is_last && n >= len - f) return __fmul_rn(x, __fdiv_rn(__fadd_rn((float)(len - 1 - n), 0.5f), (float)f));
  }
  return x;
}

__global__ __launch_bounds__(WJ_T) void wj_emit_kernel(const float* __restrict__ pieces, int64_t pitch, const int32_t* __restrict__ bounds,
                                                       const int32_t* __restrict__ first, const int32_t* __restrict__ offsets, int fade,
                                                       float* __restrict__ dst, int64_t dst_pitch, float* __restrict__ tmax, int ntile,
                                                       int L, int Lj) {
  __shared__ float sh[WJ_T / 64];
  const int p = blockIdx.x / ntile, t = blockIdx.x % ntile;
  const int lo = first[p], hi = first[p + 1];
  float* row = dst + (int64_t)p * dst_pitch;
  const int a = (int)((reinterpret_cast<uintptr_t>(row) >> 2) & 3);   // floats of the row's start behind a 16-byte boundary
  const int64_t j0 = ((int64_t)t * WJ_T + threadIdx.x) * WJ_PER - a;
  float v[WJ_PER] = {0.f, 0.f, 0.f, 0.f};
  if (j0 < Lj && hi > lo) {
    const int jf = j0 < 0 ? 0 : (int)j0;
    int i = lo, e = hi;   // the last piece with offsets[i] <= jf is in [i, e); offsets[lo] == 0
    while (e - i > 1) {
      const int mid = i + ((e - i) >> 1);
      if (offsets[mid] <= jf) i = mid; else e = mid;
    }
    int off = offsets[i], len = wj_len(bounds, i, L);
#pragma unroll
    for (int k = 0; k < WJ_PER; ++k) {
      const int64_t j = j0 + k;
      if (j < 0 || j >= Lj) continue;
      while (i + 1 < hi && offsets[i + 1] <= j) {   // (a piece that starts at Lj is under no output: offsets are clamped to Lj)
        ++i;
        off = offsets[i];
        len = wj_len(bounds, i, L);
      }
      const int n = (int)j - off;
      if (n < len) v[k] = wj_sample(pieces + (int64_t)i * pitch, n, len, fade, i == lo, i == hi - 1);
    }
  }
  if (j0 >= 0 && j0 + WJ_PER <= Lj) {
    *reinterpret_cast<float4*>(row + j0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < WJ_PER; ++k)
      if (j0 + k >= 0 && j0 + k < Lj) row[j0 + k] = v[k];
  }
  float m = fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3])));   // (outputs outside the row stayed 0)
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) tmax[(int64_t)p * ntile + t] = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}

// peak[p] = the maximum of the prompt's tile maxima; pcm by wf_emit_kernel's rule with that peak.  tiles: workgroups per prompt
// (ntile, or 1 when there is no pcm: the peak alone)
__global__ __launch_bounds__(WJ_T) void wj_pcm_kernel(const float* __restrict__ src, int64_t src_pitch, const float* __restrict__ tmax,
                                                      int ntile, int tiles, float* __restrict__ peak, int16_t* __restrict__ pcm, int Lj) {
  __shared__ float sh[WJ_T / 64];
  const int p = blockIdx.x / tiles, t = blockIdx.x % tiles;
  float m = 0.f;
  for (int k = threadIdx.x; k < ntile; k += WJ_T) m = fmaxf(m, tmax[(int64_t)p * ntile + k]);
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
  __syncthreads();
  const float pk = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
  if (t == 0 && threadIdx.x == 0) peak[p] = pk;
  if (!pcm) return;
  int16_t* row = pcm + (int64_t)p * Lj;
  const int a = (int)((reinterpret_cast<uintptr_t>(row) >> 1) & 3);   // samples of the row's start behind an 8-byte boundary
  const int64_t j0 = ((int64_t)t * WJ_T + threadIdx.x) * WJ_PER - a;
  if (j0 >= Lj) return;
  const float* x = src + (int64_t)p * src_pitch;
  int16_t q[WJ_PER] = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < WJ_PER; ++k) {
    const int64_t j = j0 + k;
    if (j < 0 || j >= Lj) continue;
    q[k] = pcm16(x[j], pk);
  }
  if (j0 >= 0 && j0 + WJ_PER <= Lj) {
    *reinterpret_cast<short4*>(row + j0) = make_short4(q[0], q[1], q[2], q[3]);
  } else {
#pragma unroll
    for (int k = 0; k < WJ_PER; ++k)
      if (j0 + k >= 0 && j0 + k < Lj) row[j0 + k] = q[k];
  }
}

}  // namespace

// ---- C ABI (include/taco_hip.h): the Griffin-Lim entry points, taco_wave_finish and taco_wave_join, each behind the one layout
// of its workspace
// Griffin-Lim: the angles, the segments, the window sum-of-squares tables (wss_rows: 1 where one table serves the batch, B where
// each row has its own, since it depends on F_b); fast adds the previous spectrum, the two (B, F) partial-sum tables and ||M||^2
// per row.
struct GlWs {
  float *ang, *seg, *wss, *tprev, *red, *mpart, *msq;
  int64_t bytes;
};
static GlWs gl_ws(void* ws, int B, int F, int wss_rows, bool fast) {
  WsCarver c(ws);
  GlWs w{};
  const int64_t BF = (int64_t)B * F;
  w.ang = c.take<float>(BF * NBIN * 2);
  w.seg = c.take<float>(BF * WIN);
  w.wss = c.take<float>(wss_rows * (NFFT + (int64_t)HOP * (F - 1)));
  if (fast) {
    w.tprev = c.take<float>(BF * NBIN * 2);
    w.red = c.take<float>(BF);
    w.mpart = c.take<float>(BF);
    w.msq = c.take<float>(B);
  }
  c.take<float>(64);   // slack, for nothing: no array is aligned beyond the base.  Callers size buffers with it.
  w.bytes = c.bytes;
  return w;
}

// F >= 5: the centre (reflect) padding of n_fft / 2 = 1024 samples at hop 300 needs more than 1024 samples
static bool griffinlim_shape_ok(int B, int F) { return B > 0 && F >= 5; }

extern "C" int64_t taco_griffinlim_workspace_bytes(int B, int F) {
  return griffinlim_shape_ok(B, F) ? gl_ws(nullptr, B, F, 1, false).bytes : TACO_EINVAL;
}
extern "C" int64_t taco_griffinlim_rows_workspace_bytes(int B, int F) {
  return griffinlim_shape_ok(B, F) ? gl_ws(nullptr, B, F, B, false).bytes : TACO_EINVAL;
}
extern "C" int64_t taco_griffinlim_fast_workspace_bytes(int B, int F) {
  return griffinlim_shape_ok(B, F) ? gl_ws(nullptr, B, F, B, true).bytes : TACO_EINVAL;
}

// What all three Griffin-Lim entry points require, in the order a caller sees the refusals.  `who`: the entry point's name in the
// messages; pointers: whether every pointer that entry point requires is non-null; momentum: 0 where there is none.
static int griffinlim_require(const char* who, bool pointers, int B, int F, int n_iter, int frames_per_unit, float momentum = 0.f) {
  TACO_REQUIRE(pointers && B > 0 && n_iter >= 0 && frames_per_unit >= 1, "%s: bad arguments", who);
  TACO_REQUIRE(momentum >= 0.f && momentum < 1.f, "%s: momentum %g is not in [0, 1)", who, (double)momentum);   // (NaN fails)
  TACO_REQUIRE(F >= 5, "%s: F=%d frames < 5 (the reflect padding of n_fft/2 needs more than 1024 samples)", who, F);
  return TACO_OK;
}

// the launches of all three entry points.  frames == nullptr: every row has F frames and one window table serves the batch.
// alpha > 0: momentum rounds with the previous spectrum in w.tprev; conv != nullptr: the readout, (B, n_iter + 1), with its
// scratch in w.red, w.mpart, w.msq.  alpha == 0 and conv == nullptr are the launches of taco_griffinlim / taco_griffinlim_rows.
static int griffinlim_launches(const float* mag_t, const float* phase0, uint64_t seed, const int32_t* frames, int per_unit,
                               float* wave, const GlWs& w, int B, int F, int n_iter, hipStream_t s, float alpha = 0.f,
                               float* conv = nullptr) {
  float *ang = w.ang, *seg = w.seg, *wss = w.wss, *red = w.red, *mpart = w.mpart, *msq = w.msq;
  const int n = NFFT + HOP * (F - 1);
  const int64_t wss_pitch = frames ? n : 0;
  const bool mom = alpha > 0.f;
  GlExtra x{mom ? w.tprev : nullptr, alpha, 0, 0, mag_t, red};
  TACO_KLAUNCH(gl_wss_kernel, dim3((n + 255) / 256, frames ? B : 1), dim3(256), 0, s, wss, wss_pitch, F, frames, per_unit);
  const int64_t total = (int64_t)B * F * NBIN;
  TACO_KLAUNCH(gl_init_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 4096)), dim3(256), 0, s, phase0, seed, ang, F,
                     total, frames, per_unit);
  if (conv) TACO_KLAUNCH(gl_magsq_kernel, dim3(F, B), dim3(FT), 0, s, mag_t, mpart, F, frames, per_unit);
  for (int it = 0; it < n_iter; ++it) {
    TACO_KLAUNCH(gl_synth_kernel, dim3(F, B), dim3(FT), 0, s, mag_t, ang, seg, F, frames, per_unit);
    x.read_prev = it > 0;
    x.write_prev = it < n_iter - 1;
    if (mom && conv)
      TACO_KLAUNCH((gl_anal_kernel<true, true, true>), dim3(F, B), dim3(FT), 0, s, seg, wss, wss_pitch, ang, F, frames, per_unit, x);
    else if (mom)
      TACO_KLAUNCH((gl_anal_kernel<true, false, true>), dim3(F, B), dim3(FT), 0, s, seg, wss, wss_pitch, ang, F, frames, per_unit, x);
    else if (conv)
      TACO_KLAUNCH((gl_anal_kernel<false, true, true>), dim3(F, B), dim3(FT), 0, s, seg, wss, wss_pitch, ang, F, frames, per_unit, x);
    else
      TACO_KLAUNCH((gl_anal_kernel<false, false, true>), dim3(F, B), dim3(FT), 0, s, seg, wss, wss_pitch, ang, F, frames, per_unit, x);
    if (conv)
      TACO_KLAUNCH(gl_conv_kernel, dim3(B), dim3(FT), 0, s, red, mpart, msq, conv, it, n_iter + 1, F, frames, per_unit, (int)(it == 0));
  }
  TACO_KLAUNCH(gl_synth_kernel, dim3(F, B), dim3(FT), 0, s, mag_t, ang, seg, F, frames, per_unit);
  if (conv) {   // the readout of the returned waveform: one more analysis pass that stores no angles
    TACO_KLAUNCH((gl_anal_kernel<false, true, false>), dim3(F, B), dim3(FT), 0, s, seg, wss, wss_pitch, ang, F, frames, per_unit, x);
    TACO_KLAUNCH(gl_conv_kernel, dim3(B), dim3(FT), 0, s, red, mpart, msq, conv, n_iter, n_iter + 1, F, frames, per_unit,
                 (int)(n_iter == 0));
  }
  TACO_KLAUNCH(gl_wave_kernel, dim3((HOP * (F - 1) + 255) / 256, B), dim3(256), 0, s, seg, wss, wss_pitch, wave, F, frames, per_unit);
  return TACO_OK;
}

extern "C" int taco_griffinlim(const float* mag_t, const float* phase0, float* wave, void* workspace, int B, int F, int n_iter,
                               void* stream) {
  TACO_TRY(griffinlim_require("griffinlim", mag_t && phase0 && wave && workspace, B, F, n_iter, 1));
  griffinlim_launches(mag_t, phase0, 0, nullptr, 1, wave, gl_ws(workspace, B, F, 1, false), B, F, n_iter, as_stream(stream));
  TACO_LAUNCH_CHECK("griffinlim");
  return TACO_OK;
}

extern "C" int taco_griffinlim_rows(const float* mag_t, const float* phase0, uint64_t seed, const int32_t* frames,
                                    int frames_per_unit, float* wave, void* workspace, int B, int F, int n_iter, void* stream) {
  TACO_TRY(griffinlim_require("griffinlim_rows", mag_t && frames && wave && workspace, B, F, n_iter, frames_per_unit));
  griffinlim_launches(mag_t, phase0, seed, frames, frames_per_unit, wave, gl_ws(workspace, B, F, B, false), B, F, n_iter,
                      as_stream(stream));
  TACO_LAUNCH_CHECK("griffinlim_rows");
  return TACO_OK;
}

extern "C" int taco_griffinlim_fast(const float* mag_t, const float* phase0, uint64_t seed, const int32_t* frames,
                                    int frames_per_unit, float momentum, float* wave, float* conv, void* workspace, int B, int F,
                                    int n_iter, void* stream) {
  TACO_TRY(griffinlim_require("griffinlim_fast", mag_t && wave && workspace, B, F, n_iter, frames_per_unit, momentum));
  TACO_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "griffinlim_fast: workspace is not 8-byte aligned");
  griffinlim_launches(mag_t, phase0, seed, frames, frames_per_unit, wave, gl_ws(workspace, B, F, B, true), B, F, n_iter,
                      as_stream(stream), momentum, conv);
  TACO_LAUNCH_CHECK("griffinlim_fast");
  return TACO_OK;
}

// workspace of taco_wave_finish: y (B, L rounded up to 4), the chunk aggregates, the 512-sample maxima, the trim frames' mean
// squares
static int64_t wf_pitch(int L) { return ((int64_t)L + 3) & ~(int64_t)3; }
static int wf_chunks(int L) { return cdiv(L, WF_CHUNK); }
static int wf_blocks(int L) { return cdiv(L, 512); }
static int wf_frames(int L) { return 1 + L / TRIM_HOP; }
struct WfWs {
  float *y, *agg, *pm, *ms;
  int64_t bytes;
};
static WfWs wf_ws(void* ws, int B, int L) {
  WsCarver c(ws, 16);   // y is read by 16 bytes: the base is rounded up
  WfWs w;
  w.y = c.take<float>(B * wf_pitch(L));
  w.agg = c.take<float>((int64_t)B * wf_chunks(L));
  w.pm = c.take<float>((int64_t)B * wf_blocks(L));
  w.ms = c.take<float>((int64_t)B * wf_frames(L));
  c.take<float>(64);   // slack: the up to 15 bytes that rounding the base up costs
  w.bytes = c.bytes;
  return w;
}
extern "C" int64_t taco_wave_finish_workspace_bytes(int B, int L) {
  if (B <= 0 || L <= 0) return TACO_EINVAL;
  return wf_ws(nullptr, B, L).bytes;
}

extern "C" int taco_wave_finish(const float* wave, const int32_t* samples, float deemphasis, float trim_top_db, float* out,
                                int16_t* pcm, int32_t* bounds, float* peak, void* workspace, int B, int L, void* stream) {
  TACO_REQUIRE(wave && bounds && peak && workspace && B > 0 && L > 0, "wave_finish: bad arguments");
  TACO_REQUIRE(out || pcm, "wave_finish: out and pcm are both NULL");
  TACO_REQUIRE(out != wave, "wave_finish: out may not alias wave (the emit pass shifts by the trim start)");
  TACO_REQUIRE(deemphasis >= 0.f && deemphasis < 1.f, "wave_finish: deemphasis %g is not in [0, 1)", (double)deemphasis);   // (NaN fails)
  TACO_REQUIRE(trim_top_db >= 0.f, "wave_finish: trim_top_db %g is negative or NaN", (double)trim_top_db);
  hipStream_t s = as_stream(stream);
  const int64_t pitch = wf_pitch(L);
  const int nch = wf_chunks(L), npm = wf_blocks(L), nms = wf_frames(L);
  const WfWs w = wf_ws(workspace, B, L);
  float *y = w.y, *agg = w.agg, *pm = w.pm, *ms = w.ms;
  if (deemphasis != 0.f && nch > 1)
    TACO_KLAUNCH((wf_scan_kernel<true>), dim3(nch - 1, B), dim3(WF_T), 0, s, wave, samples, deemphasis, y, pitch, agg, nch, pm, npm, L);
  TACO_KLAUNCH((wf_scan_kernel<false>), dim3(nch, B), dim3(WF_T), 0, s, wave, samples, deemphasis, y, pitch, agg, nch, pm, npm, L);
  if (trim_top_db > 0.f)
    TACO_KLAUNCH(wf_ms_kernel, dim3(cdiv(nms, WF_T / 64), B), dim3(WF_T), 0, s, y, pitch, samples, ms, nms, L);
  TACO_KLAUNCH(wf_bounds_kernel, dim3(B), dim3(WF_BT), 0, s, ms, nms, pm, npm, samples, trim_top_db, bounds, peak, L);
  TACO_KLAUNCH(wf_emit_kernel, dim3(std::min(cdiv(L, 1024), 2048), B), dim3(256), 0, s, y, pitch, bounds, peak, out, pcm, L);
  TACO_LAUNCH_CHECK("wave_finish");
  return TACO_OK;
}

// workspace of taco_wave_join: the joined fp32 rows (P, Lj rounded up to 4; used when out is NULL), the tile maxima, the device copies
// of first and gap
static int64_t wj_pitch(int Lj) { return ((int64_t)Lj + 3) & ~(int64_t)3; }
static int wj_tiles(int Lj) { return cdiv(cdiv((int64_t)Lj + 3, WJ_PER), WJ_T); }   // chunks of a row at its worst alignment
struct WjWs {
  float *rows, *tmax;
  int32_t *first, *gap;
  int64_t bytes;
};
static WjWs wj_ws(void* ws, int N, int P, int Lj) {
  WsCarver c(ws, 16);   // the rows are written by 16 bytes: the base is rounded up
  WjWs w;
  w.rows = c.take<float>(P * wj_pitch(Lj));
  w.tmax = c.take<float>((int64_t)P * wj_tiles(Lj));
  w.first = c.take<int32_t>((int64_t)P + 1);
  w.gap = c.take<int32_t>(N);
  c.take<char>(64);   // slack: the up to 15 bytes that rounding the base up costs
  w.bytes = c.bytes;
  return w;
}
extern "C" int64_t taco_wave_join_workspace_bytes(int N, int P, int Lj) {
  if (N <= 0 || P <= 0 || Lj <= 0) return TACO_EINVAL;
  return wj_ws(nullptr, N, P, Lj).bytes;
}

extern "C" int taco_wave_join(const float* pieces, int64_t pitch, const int32_t* bounds, const int32_t* first, const int32_t* gap,
                              int fade, float* out, int16_t* pcm, int32_t* offsets, int32_t* total, float* peak, void* workspace,
                              int N, int P, int L, int Lj, void* stream) {
  TACO_REQUIRE(pieces && bounds && first && gap && offsets && total && peak && workspace, "wave_join: null pointer");
  TACO_REQUIRE(out || pcm, "wave_join: out and pcm are both NULL");
  TACO_REQUIRE(N > 0 && P > 0 && L > 0 && Lj > 0, "wave_join: N=%d P=%d L=%d Lj=%d", N, P, L, Lj);
  TACO_REQUIRE(pitch >= L, "wave_join: pitch %lld is below L=%d", (long long)pitch, L);
  TACO_REQUIRE(fade >= 0, "wave_join: fade %d is negative", fade);
  TACO_REQUIRE(!out || !bytes_meet(out, (uint64_t)P * (uint64_t)Lj * 4, pieces, (((uint64_t)N - 1) * (uint64_t)pitch + (uint64_t)L) * 4),
               "wave_join: out overlaps pieces");
  TACO_REQUIRE(first[0] == 0 && first[P] == N, "wave_join: first[0]=%d, first[P]=%d: they must be 0 and N=%d", first[0], first[P], N);
  for (int p = 0; p < P; ++p)
    TACO_REQUIRE(first[p] <= first[p + 1], "wave_join: first[%d]=%d is above first[%d]=%d", p, first[p], p + 1, first[p + 1]);
  for (int i = 0; i < N; ++i) TACO_REQUIRE(gap[i] >= 0, "wave_join: gap[%d]=%d is negative", i, gap[i]);
  const int ntile = wj_tiles(Lj);
  TACO_REQUIRE((int64_t)P * ntile <= 0x7fffffff, "wave_join: P=%d prompts of %d tiles are more than one grid holds", P, ntile);
  hipStream_t s = as_stream(stream);
  const int64_t rpitch = wj_pitch(Lj);
  const WjWs w = wj_ws(workspace, N, P, Lj);
  float *rows = w.rows, *tmax = w.tmax;
  int32_t *first_d = w.first, *gap_d = w.gap;
  TACO_TRY(taco_upload_async(first_d, first, ((size_t)P + 1) * sizeof(int32_t), s, "wave_join: first upload"));
  TACO_TRY(taco_upload_async(gap_d, gap, (size_t)N * sizeof(int32_t), s, "wave_join: gap upload"));
  float* dst = out ? out : rows;
  const int64_t dst_pitch = out ? (int64_t)Lj : rpitch;
  const int tiles = pcm ? ntile : 1;
  TACO_KLAUNCH(wj_offsets_kernel, dim3(P), dim3(WJ_T), 0, s, bounds, first_d, gap_d, offsets, total, L, Lj);
  TACO_KLAUNCH(wj_emit_kernel, dim3((unsigned)((int64_t)P * ntile)), dim3(WJ_T), 0, s, pieces, pitch, bounds, first_d, offsets, fade,
               dst, dst_pitch, tmax, ntile, L, Lj);
  TACO_KLAUNCH(wj_pcm_kernel, dim3((unsigned)((int64_t)P * tiles)), dim3(WJ_T), 0, s, dst, dst_pitch, tmax, ntile, tiles, peak, pcm, Lj);
  TACO_LAUNCH_CHECK("wave_join");
  return TACO_OK;
}
