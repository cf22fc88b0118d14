// features.hip -- training features from waveforms on the GPU (audio.process_audio, audio.py:38-65; the producer half of
// preprocess.py).  The reference's constants are compiled in, as in vocoder.hip: n_fft 2048, win_length 1200 (periodic Hann,
// zero-padded to 2048 around its centre), hop 300, pre-emphasis 0.97, log(|.| + 1e-8).  Per utterance, in the reference's order:
//
//   1. trim     librosa.effects.trim(wave) with its defaults, in the librosa 0.6 form: the mean square of frames of 2048
//               samples at hop 512 of the signal reflect-padded by 1024; a frame is non-silent when
//               10 log10(max(1e-10, ms)) - 10 log10(max(1e-10, max ms)) > -60; start = 512 first, end = min(len, 512 (last + 1)).
//               (librosa 0.5 took the RMS from STFT magnitudes instead; the reference pins no librosa release.)  An all-zero
//               wave is all 0 dB and is not trimmed.
//   2. drop / pad  end - start > max_len: dropped (the reference's `return None, None`); else zero-padded to max_len.  The
//               padding is index arithmetic in the frame gather, no copy.
//   3. pre-emphasis after the padding: e[0] = y[0], e[n] = y[n] - 0.97 y[n - 1] (so the first padded sample is -0.97 y[end-1]).
//   4. STFT     center=True (reflect padding by 1024), F = 1 + max_len / 300 frames, 1025 bins -> log(|X| + 1e-8).
//   5. mel      librosa.feature.melspectrogram(S=stft, n_mels=80) with S COMPLEX and sr left at 22050: |M X|, the filterbank
//               applied to the complex bins (not to power, not to magnitudes) -> log(|M X| + 1e-8).  M (80, 1025) comes from the
//               host (audio.mel_basis); each row is a triangle and only its nonzero run of bins is summed.
//   6. r-frame layout written in place (audio.reshape_frames): frame f = 4rc + 4i + j -> row 4c + j, column block i; only the
//               first (F / 4r) 4r frames, as reshape_frames keeps.
//
// Launches: fb_ranges (the nonzero run of every filterbank row), fb_trim (one workgroup per utterance: frame energies into the
// workspace, then the bounds and the keep flag), fb_frames (steps 2-6: a grid-stride run of frames per workgroup, so the twiddle
// table and the window are built once per workgroup).  Each frame is ONE real 2048-point FFT done as a 1024-point complex FFT of
// its even / odd samples plus the Hermitian split.  Two different frames are deliberately not packed into one complex FFT: the
// split leaks the rounding error of one frame into the other, and next to the trimmed end a frame holding a single window-edge
// sample sits 1e-6 below its neighbour -- its own spectrum would be lost in the leak.  No atomics: every sum has a fixed order,
// two calls give identical bits.
#include <hip/hip_fp16.h>

#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int NFFT = 2048, NBIN = 1025, WIN = 1200, HOP = 300, WOFF = (NFFT - WIN) / 2;   // window occupies [424, 1624)
constexpr int NH = NFFT / 2;                  // 1024-point complex FFT of the even / odd samples
constexpr int NMEL = 80;
constexpr int FT = 256;                       // fb_frames block
constexpr int TT = 512;                       // fb_trim block
constexpr int TRIM_FRAME = 2048, TRIM_HOP = 512;
constexpr float PREEMPH = 0.97f, LOG_EPS = 1e-8f;

// LDS index with one pad word per 32: the radix-2 stages' stride-2 (first stage) and stride-2^s accesses spread over the 32
// banks of ds_read_b32 / ds_write_b32 (cdna_hip_programming.md Guideline 4)
__device__ __forceinline__ int pd(int i) { return i + (i >> 5); }
constexpr int NH_PAD = NH + NH / 32;

__device__ __forceinline__ int bitrev10(int x) { return (int)(__brev((unsigned)x) >> 22); }

// numpy.pad(mode='reflect') index for any pad width: period 2 (n - 1)
__device__ __forceinline__ int64_t reflect_any(int64_t p, int64_t n) {
  if (n <= 1) return 0;
  const int64_t per = 2 * (n - 1);
  int64_t q = p % per;
  if (q < 0) q += per;
  return q >= n ? per - q : q;
}

// nonzero run [lo, hi) of every filterbank row: one wave per row
__global__ __launch_bounds__(256) void fb_ranges_kernel(const float* __restrict__ basis, int* __restrict__ rng) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int m = w; m < NMEL; m += 4) {
    float lo = -(float)NBIN, hi = -1.f;   // as maxima: lo holds -first, hi holds last
    for (int k = lane; k < NBIN; k += 64)
      if (basis[m * NBIN + k] != 0.f) {
        lo = fmaxf(lo, -(float)k);
        hi = fmaxf(hi, (float)k);
      }
    lo = wave_max(lo);
    hi = wave_max(hi);
    if (lane == 0) {
      const int l = (int)(-lo), h = (int)hi + 1;
      rng[2 * m] = h > 0 ? l : 0;
      rng[2 * m + 1] = h > 0 ? h : 0;
    }
  }
}

// one workgroup per utterance: ms[t] for the 1 + n / 512 trim frames (each wave its own frames), then the bounds
__global__ __launch_bounds__(TT) void fb_trim_kernel(const float* __restrict__ wave, const int* __restrict__ wave_len,
                                                     float* __restrict__ ms_all, int64_t ms_stride, int* __restrict__ bounds,
                                                     int* __restrict__ kept, int L, int max_len) {
  constexpr int NW = TT / 64;
  __shared__ float red_max[NW];
  __shared__ int red_lo[NW], red_hi[NW];
  const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int n = wave_len[b];
  const int nt = 1 + n / TRIM_HOP;
  const float* x = wave + (int64_t)b * L;
  float* ms = ms_all + (int64_t)b * ms_stride;
  float mx = 0.f;
  for (int t = w; t < nt; t += NW) {
    float acc = 0.f;
    for (int i = lane; i < TRIM_FRAME; i += 64) {
      const float v = x[reflect_any((int64_t)t * TRIM_HOP + i - TRIM_FRAME / 2, n)];
      acc = fmaf(v, v, acc);
    }
    const float m = wave_sum(acc) * (1.0f / TRIM_FRAME);
    if (lane == 0) ms[t] = m;   // read back below by this same wave only
    mx = fmaxf(mx, m);
  }
  if (lane == 0) red_max[w] = mx;
  __syncthreads();
  mx = red_max[0];
  for (int i = 1; i < NW; ++i) mx = fmaxf(mx, red_max[i]);
  const float ref_db = 10.f * log10f(fmaxf(1e-10f, mx));
  int lo = 0x7fffffff, hi = -1;
  if (lane == 0)
    for (int t = w; t < nt; t += NW)
      if (10.f * log10f(fmaxf(1e-10f, ms[t])) - ref_db > -60.f) {
        lo = min(lo, t);
        hi = max(hi, t);
      }
  if (lane == 0) {
    red_lo[w] = lo;
    red_hi[w] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 0; i < NW; ++i) {
      lo = min(lo, red_lo[i]);
      hi = max(hi, red_hi[i]);
    }
    int start = 0, end = 0;   // (no non-silent frame: only a NaN wave gets here; librosa returns the empty slice)
    if (hi >= 0) {
      start = lo * TRIM_HOP;
      end = min(n, (hi + 1) * TRIM_HOP);
    }
    bounds[2 * b] = start;
    bounds[2 * b + 1] = end;
    kept[b] = (end - start <= max_len) ? 1 : 0;
  }
}

struct FrameArgs {
  const float* wave;
  const float* basis;
  const int* rng;
  const int* bounds;
  const int* kept;
  void* mel;
  void* stft;
  int L, max_len, r, Fk, Td, B, fp16;
};

__device__ __forceinline__ void store_out(void* base, int64_t i, float v, int fp16) {
  if (fp16) static_cast<__half*>(base)[i] = __float2half_rn(v);
  else static_cast<float*>(base)[i] = v;
}

__global__ __launch_bounds__(FT) void fb_frames_kernel(FrameArgs a) {
  __shared__ float zr[NH_PAD], zi[NH_PAD];   // the 1024-point complex FFT (bit-reversed load, in place)
  __shared__ float xr[NBIN], xi[NBIN];       // the frame's 1025 complex bins
  __shared__ float twr[NH], twi[NH];         // e^{-2 pi i k / 2048}, k < 1024
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int k = tid; k < NH; k += FT) {
    float s, c;
    sincospif(-2.0f * (float)k / (float)NFFT, &s, &c);
    twr[k] = c;
    twi[k] = s;
  }
  // this thread's input samples: j = 2n (real part) and 2n + 1 (imaginary part) for n = tid + FT u; their window values
  float win[2 * (NH / FT)];
#pragma unroll
  for (int u = 0; u < NH / FT; ++u)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int j = 2 * (tid + FT * u) + h;
      float s, c;
      sincospif(2.0f * (float)(j - WOFF) / (float)WIN, &s, &c);
      win[2 * u + h] = (j >= WOFF && j < WOFF + WIN) ? 0.5f - 0.5f * c : 0.f;
    }
  const int64_t total = (int64_t)a.B * a.Fk;
  const int rc = 4 * a.r;
  const int64_t srow = (int64_t)NBIN * a.r, mrow = (int64_t)NMEL * a.r;
  for (int64_t g = blockIdx.x; g < total; g += gridDim.x) {
    const int b = (int)(g / a.Fk), f = (int)(g - (int64_t)b * a.Fk);
    const int c = f / rc, i = (f - c * rc) >> 2, jr = f & 3;
    const int64_t row = (int64_t)b * a.Td + 4 * c + jr;
    const int64_t so = row * srow + (int64_t)i * NBIN, mo = row * mrow + (int64_t)i * NMEL;
    if (!a.kept[b]) {   // dropped utterance: zero rows (uniform over the workgroup)
      for (int k = tid; k < NBIN; k += FT) store_out(a.stft, so + k, 0.f, a.fp16);
      for (int m = tid; m < NMEL; m += FT) store_out(a.mel, mo + m, 0.f, a.fp16);
      continue;
    }
    const int start = a.bounds[2 * b];
    const int lt = a.bounds[2 * b + 1] - start;   // trimmed length <= max_len: samples [lt, max_len) are the zero padding
    const float* y = a.wave + (int64_t)b * a.L + start;
    __syncthreads();   // (previous frame's readers of zr / xr are done)
#pragma unroll
    for (int u = 0; u < NH / FT; ++u) {
      const int n = tid + FT * u;
      float v[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int j = 2 * n + h;
        float e = 0.f;
        if (win[2 * u + h] != 0.f) {
          int q = f * HOP + j - NFFT / 2;         // centre padding: reflect into [0, max_len)
          if (q < 0) q = -q;
          if (q >= a.max_len) q = 2 * (a.max_len - 1) - q;
          const float y0 = q < lt ? y[q] : 0.f;   // zero padding to max_len, as index arithmetic
          const float y1 = (q > 0 && q - 1 < lt) ? y[q - 1] : 0.f;
          e = q == 0 ? y0 : fmaf(-PREEMPH, y1, y0);
        }
        v[h] = e * win[2 * u + h];
      }
      const int p = pd(bitrev10(n));
      zr[p] = v[0];
      zi[p] = v[1];
    }
#pragma unroll 1
    for (int s = 0; s < 10; ++s) {
      const int half = 1 << s;
      __syncthreads();
      for (int t = tid; t < NH / 2; t += FT) {
        const int pos = t & (half - 1);
        const int i0 = ((t >> s) << (s + 1)) + pos, i1 = i0 + half;
        const int k = pos << (10 - s);   // W_1024^(pos 512 / half) = W_2048^(pos 1024 / half)
        const float wr = twr[k], wi = twi[k];
        const int p0 = pd(i0), p1 = pd(i1);
        const float ar = zr[p1], ai = zi[p1];
        const float tr = ar * wr - ai * wi, ti = ar * wi + ai * wr;
        const float ur = zr[p0], ui = zi[p0];
        zr[p0] = ur + tr; zi[p0] = ui + ti;
        zr[p1] = ur - tr; zi[p1] = ui - ti;
      }
    }
    __syncthreads();
    // Hermitian split: Z = E' + i O' (E', O' the FFTs of the even / odd samples); X[k] = E'[k] + W_2048^k O'[k]
    for (int k = tid; k < NBIN; k += FT) {
      const int k0 = k & (NH - 1), k1 = (NH - k) & (NH - 1);
      const float ar = zr[pd(k0)], ai = zi[pd(k0)];
      const float br = zr[pd(k1)], bi = -zi[pd(k1)];   // conj Z[N/2 - k]
      const float er = 0.5f * (ar + br), ei = 0.5f * (ai + bi);
      const float orr = 0.5f * (ai - bi), oi = -0.5f * (ar - br);   // (a - b) / 2i
      const float wr = k < NH ? twr[k] : -1.f, wi = k < NH ? twi[k] : 0.f;
      const float Xr = er + (orr * wr - oi * wi), Xi = ei + (orr * wi + oi * wr);
      xr[k] = Xr;
      xi[k] = Xi;
      store_out(a.stft, so + k, logf(sqrtf(Xr * Xr + Xi * Xi) + LOG_EPS), a.fp16);
    }
    __syncthreads();
    // mel: |sum_k M[m, k] X[k]| over the row's nonzero run; one wave per row, lanes stride the run, fixed-order wave sums
    for (int m = w; m < NMEL; m += FT / 64) {
      const int lo = a.rng[2 * m], hi = a.rng[2 * m + 1];
      const float* bm = a.basis + (int64_t)m * NBIN;
      float sr = 0.f, si = 0.f;
      for (int k = lo + lane; k < hi; k += 64) {
        const float c0 = bm[k];
        sr = fmaf(c0, xr[k], sr);
        si = fmaf(c0, xi[k], si);
      }
      sr = wave_sum(sr);
      si = wave_sum(si);
      if (lane == 0) store_out(a.mel, mo + m, logf(sqrtf(sr * sr + si * si) + LOG_EPS), a.fp16);
    }
  }
}

struct FeatWs {
  int64_t len, rng, ms, ms_stride, bytes;
};
FeatWs feat_ws(int B, int L) {
  FeatWs w;
  auto up = [](int64_t x) { return (x + 255) & ~(int64_t)255; };
  w.len = 0;
  w.rng = up((int64_t)B * 4);
  w.ms = w.rng + up(2 * NMEL * 4);
  w.ms_stride = 1 + (int64_t)L / TRIM_HOP;
  w.bytes = w.ms + up((int64_t)B * w.ms_stride * 4);
  return w;
}

}  // namespace

// ---- C ABI (include/taco_hip.h)
extern "C" int64_t taco_audio_features_workspace_bytes(int B, int L) {
  if (B <= 0 || L <= 0) return TACO_EINVAL;
  return feat_ws(B, L).bytes;
}

extern "C" int taco_audio_features(const float* wave, const int* wave_len_host, const float* mel_basis, void* mel, void* stft,
                                   int* bounds, int* kept, void* workspace, int B, int L, int max_len, int r, int out_fp16,
                                   void* stream) {
  TACO_REQUIRE(wave && wave_len_host && mel_basis && mel && stft && bounds && kept && workspace,
               "audio_features: null pointer");
  TACO_REQUIRE(B > 0 && L > 0, "audio_features: B=%d L=%d", B, L);
  TACO_REQUIRE(r >= 1 && r <= 5, "audio_features: r=%d outside 1..5", r);
  TACO_REQUIRE(out_fp16 == 0 || out_fp16 == 1, "audio_features: out_fp16=%d (0 or 1)", out_fp16);
  TACO_REQUIRE(max_len > 0 && max_len % HOP == 0, "audio_features: max_len=%d is not a positive multiple of %d", max_len, HOP);
  const int F = 1 + max_len / HOP;
  TACO_REQUIRE(max_len > NFFT / 2 && F >= 4 * r,
               "audio_features: max_len=%d gives %d frames, fewer than one chunk of 4r=%d (or too short to reflect-pad by %d)",
               max_len, F, 4 * r, NFFT / 2);
  for (int b = 0; b < B; ++b)
    TACO_REQUIRE(wave_len_host[b] >= 1 && wave_len_host[b] <= L, "audio_features: wave_len[%d]=%d outside 1..L=%d", b,
                 wave_len_host[b], L);
  hipStream_t s = as_stream(stream);
  const FeatWs W = feat_ws(B, L);
  char* ws = static_cast<char*>(workspace);
  int* len_d = reinterpret_cast<int*>(ws + W.len);
  int* rng = reinterpret_cast<int*>(ws + W.rng);
  float* ms = reinterpret_cast<float*>(ws + W.ms);
  TACO_TRY(taco_upload_async(len_d, wave_len_host, (size_t)B * sizeof(int), s, "audio_features: length upload"));
  TACO_KLAUNCH(fb_ranges_kernel, dim3(1), dim3(256), 0, s, mel_basis, rng);
  TACO_KLAUNCH(fb_trim_kernel, dim3(B), dim3(TT), 0, s, wave, len_d, ms, W.ms_stride, bounds, kept, L, max_len);
  FrameArgs a;
  a.wave = wave;
  a.basis = mel_basis;
  a.rng = rng;
  a.bounds = bounds;
  a.kept = kept;
  a.mel = mel;
  a.stft = stft;
  a.L = L;
  a.max_len = max_len;
  a.r = r;
  a.Fk = (F / (4 * r)) * 4 * r;
  a.Td = a.Fk / r;
  a.B = B;
  a.fp16 = out_fp16;
  const int64_t total = (int64_t)B * a.Fk;
  TACO_KLAUNCH(fb_frames_kernel, dim3((unsigned)std::min<int64_t>(total, 2048)), dim3(FT), 0, s, a);
  TACO_LAUNCH_CHECK("audio_features");
  return TACO_OK;
}
