// stft.h -- the device numerics that the feature front end (features.hip) and the vocoder / waveform finishing (vocoder.hip) share:
// the reference's STFT constants and window, the radix-2 stages of the in-LDS FFTs, numpy's reflect index, the energy-trim rule of
// librosa.effects.trim and write_wav's PCM16 rule.  Device and constexpr code only; every function is inlined into its caller, so
// a change here changes both files' kernels alike -- these are the bits the audio tests pin.
#pragma once
#include "common.h"

constexpr int NFFT = 2048, NBIN = 1025, WIN = 1200, HOP = 300, WOFF = (NFFT - WIN) / 2;   // window occupies [424, 1624)
constexpr int FT = 256;                                // threads of a workgroup that runs an FFT
constexpr int TRIM_FRAME = 2048, TRIM_HOP = 512;       // librosa.effects.trim's defaults

__device__ __forceinline__ float hann(int i) {   // periodic Hann(1200), i in [0, 1200)
  float s, c;
  sincospif(2.0f * (float)i / (float)WIN, &s, &c);
  return 0.5f - 0.5f * c;
}

// tw[k] = e^{-2 pi i k / 2048}, k < 1024, by the FT threads of the workgroup
__device__ __forceinline__ void make_twiddles(float* twr, float* twi) {
  for (int k = threadIdx.x; k < NFFT / 2; k += FT) {
    float s, c;
    sincospif(-2.0f * (float)k / (float)NFFT, &s, &c);
    twr[k] = c;
    twi[k] = s;
  }
}

template <int BITS>
__device__ __forceinline__ int bitrev(int x) { return (int)(__brev((unsigned)x) >> (32 - BITS)); }

// LDS index maps of fft_stages: plain, or one pad word per 32 so that the stages' stride-2 (first stage) and stride-2^s accesses
// spread over the 32 banks of ds_read_b32 / ds_write_b32
struct LdsPlain {
  __device__ __forceinline__ int operator()(int i) const { return i; }
};
struct LdsPad32 {
  __device__ __forceinline__ int operator()(int i) const { return i + (i >> 5); }
};

// the STAGES in-place radix-2 stages of a 2^STAGES-point FFT of (re, im) in LDS, element i at index at(i); the data must already
// be in bit-reversed order.  sign = -1 forward, +1 inverse (unscaled).  STAGES is 11 (2048 points) or 10 (the 1024-point FFT of
// a frame's even / odd samples): the twiddle W_2048^(pos 1024 / half) is the same table entry for both.  Every stage begins with
// a barrier; the one behind the last stage is the caller's.
template <int STAGES, class At>
__device__ __forceinline__ void fft_stages(float* re, float* im, const float* twr, const float* twi, float sign, At at) {
#pragma unroll 1
  for (int s = 0; s < STAGES; ++s) {
    const int half = 1 << s;
    __syncthreads();
    for (int j = threadIdx.x; j < (1 << STAGES) / 2; j += FT) {
      const int pos = j & (half - 1);
      const int i0 = ((j >> s) << (s + 1)) + pos, i1 = i0 + half;
      const int k = pos << (10 - s);
      const float wr = twr[k], wi = -sign * twi[k];   // twi holds sin(-2 pi k / N): forward uses it as is
      const int p0 = at(i0), p1 = at(i1);
      const float xr = re[p1], xi = im[p1];
      const float tr = xr * wr - xi * wi, ti = xr * wi + xi * wr;
      const float ur = re[p0], ui = im[p0];
      re[p0] = ur + tr; im[p0] = ui + ti;
      re[p1] = ur - tr; im[p1] = ui - ti;
    }
  }
}

// numpy.pad(mode='reflect') index for any pad width: period 2 (n - 1)
__device__ __forceinline__ int64_t reflect_index(int64_t p, int64_t n) {
  if (n <= 1) return 0;
  const int64_t per = 2 * (n - 1);
  int64_t q = p % per;
  if (q < 0) q += per;
  return q >= n ? per - q : q;
}

// ---- librosa.effects.trim (the librosa 0.6 form): frames of 2048 samples at hop 512 of the row reflect-padded by 1024
// mean square of trim frame t of the n >= 1 samples of x, by one wave (every lane gets it): lane-strided, then the wave sum
__device__ __forceinline__ float trim_frame_ms(const float* __restrict__ x, int n, int t, int lane) {
  float acc = 0.f;
  for (int i = lane; i < TRIM_FRAME; i += 64) {
    const int64_t p = (int64_t)t * TRIM_HOP + i - TRIM_FRAME / 2;
    const float v = x[p >= 0 && p < n ? (int)p : (int)reflect_index(p, n)];
    acc = fmaf(v, v, acc);
  }
  return wave_sum(acc) * (1.0f / TRIM_FRAME);
}
__device__ __forceinline__ float trim_db(float ms) { return 10.f * log10f(fmaxf(1e-10f, ms)); }
// a frame is non-silent when it lies less than top_db below the loudest one (ref_db = trim_db of the largest mean square)
__device__ __forceinline__ bool trim_pass(float ms, float ref_db, float top_db) { return trim_db(ms) - ref_db > -top_db; }
// first / last non-silent frame -> [start, end); hi < 0 (no frame passes: only non-finite samples do that): the empty slice
__device__ __forceinline__ void trim_bounds(int lo, int hi, int n, int& start, int& end) {
  start = end = 0;
  if (hi >= 0) {
    start = lo * TRIM_HOP;
    end = min(n, (hi + 1) * TRIM_HOP);
  }
}

// write_wav's rule in fp32: trunc(32767 (peak > 1 ? v / peak : v)), one rounded division, one rounded multiply
__device__ __forceinline__ int16_t pcm16(float v, float peak) {
  return (int16_t)(int)truncf(__fmul_rn(peak > 1.f ? __fdiv_rn(v, peak) : v, 32767.0f));
}
