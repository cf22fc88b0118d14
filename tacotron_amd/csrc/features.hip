// features.hip -- training features from waveforms on the GPU (audio.process_audio, audio.py:38-65; the producer half of
// preprocess.py).  The reference's constants are compiled in (stft.h, with vocoder.hip): n_fft 2048, win_length 1200 (periodic Hann,
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

#include "kernels.h"
#include "stft.h"

namespace {

constexpr int NH = NFFT / 2;                  // 1024-point complex FFT of the even / odd samples
constexpr int NMEL = 80;
constexpr int TT = 512;                       // fb_trim block (fb_frames runs stft.h's FT threads)
constexpr float PREEMPH = 0.97f, LOG_EPS = 1e-8f;

constexpr int NH_PAD = NH + NH / 32;          // zr / zi carry one pad word per 32 (cdna_hip_programming.md Guideline 4)

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
    const float m = trim_frame_ms(x, n, t, lane);
    if (lane == 0) ms[t] = m;   // read back below by this same wave only
    mx = fmaxf(mx, m);
  }
  if (lane == 0) red_max[w] = mx;
  __syncthreads();
  mx = red_max[0];
  for (int i = 1; i < NW; ++i) mx = fmaxf(mx, red_max[i]);
  const float ref_db = trim_db(mx);
  int lo = 0x7fffffff, hi = -1;
  if (lane == 0)
    for (int t = w; t < nt; t += NW)
      if (trim_pass(ms[t], ref_db, 60.f)) {
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
    int start, end;
    trim_bounds(lo, hi, n, start, end);
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
  constexpr LdsPad32 pd;
  make_twiddles(twr, twi);
  // this thread's input samples: j = 2n (real part) and 2n + 1 (imaginary part) for n = tid + FT u; their window values
  float win[2 * (NH / FT)];
#pragma unroll
  for (int u = 0; u < NH / FT; ++u)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int j = 2 * (tid + FT * u) + h;
      const float hw = hann(j - WOFF);   // (evaluated for every j: a select, no divergent branch)
      win[2 * u + h] = (j >= WOFF && j < WOFF + WIN) ? hw : 0.f;
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
      const int p = pd(bitrev<10>(n));
      zr[p] = v[0];
      zi[p] = v[1];
    }
    fft_stages<10>(zr, zi, twr, twi, -1.0f, pd);
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

// workspace of taco_audio_features: the device copy of the lengths, the filterbank's bin ranges, the trim frames' mean squares,
// each on a 256-byte boundary
struct FeatWs {
  int *len, *rng;
  float* ms;
  int64_t ms_stride, bytes;
};
FeatWs feat_ws(void* ws, int B, int L) {
  WsCarver c(ws);
  FeatWs w;
  w.ms_stride = 1 + (int64_t)L / TRIM_HOP;
  w.len = c.take<int>(B, 256);
  w.rng = c.take<int>(2 * NMEL, 256);
  w.ms = c.take<float>(B * w.ms_stride, 256);
  c.take<char>(0, 256);   // the size is a whole number of 256-byte blocks
  w.bytes = c.bytes;
  return w;
}

}  // namespace

// ---- C ABI (include/taco_hip.h)
extern "C" int64_t taco_audio_features_workspace_bytes(int B, int L) {
  if (B <= 0 || L <= 0) return TACO_EINVAL;
  return feat_ws(nullptr, B, L).bytes;
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
  const FeatWs W = feat_ws(workspace, B, L);
  int *len_d = W.len, *rng = W.rng;
  float* ms = W.ms;
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

// ---- PCM decode and kaiser_best resampling (taco_hip.h taco_wave_resample): the stage in front of the feature kernels -----------
// A workgroup owns RS_TILE consecutive outputs of one row.  With first = (t0 P) / Q - (n_left - 1) the tile reads the frames
// [first, first + span): it decodes them (and mixes the channels down) straight into LDS, frames outside [0, n_orig) as 0 -- the
// clipping of the two dot products by the row's ends IS this zero extension (0 w = 0, s + 0 = s, exactly).  In signal order the K =
// n_left + n_right taps of phase p are g[m] = taps[p][n_left - 1 - m] (m < n_left: the left wing, x[nn - i]) and taps[p][m] (the right
// wing, x[nn + 1 + k]), and output t is sum_m g[m] x[nn - (n_left - 1) + m], one fp32 chain in that order.
//   UNI (Q == 1): every output has phase 0 and nn = t P, so a tap is wave-uniform (an LDS broadcast of the row staged in signal
//     order) and serves the RS_TILE / RS_BLOCK outputs of a lane.  LDS holds the span de-interleaved into P planes (frame u ->
//     plane u % P, slot u / P): lanes with consecutive outputs then read consecutive words for every tap, whatever P is.
//   otherwise the lanes of a wave have different phases: plain LDS layout, each lane reads its own tap row through L2.
constexpr int RS_TILE = TACO_WAVE_RESAMPLE_TILE, RS_BLOCK = 256, RS_PER = RS_TILE / RS_BLOCK;
constexpr int64_t RS_LDS_MAX = 64 * 1024;

namespace {

struct ResampleArgs {
  const uint8_t* pcm;
  const int32_t* rows;
  const float* taps;
  float* wave;
  int64_t row_bytes;
  int width, channels, P, Q, n_left, n_right, L, plane;   // plane: floats per LDS plane (UNI)
};

// one channel of one frame, audio.load_wav's arithmetic: 8-bit (u - 128) / 128; 16 / 32-bit float(v) 2^-(bits - 1) (int -> float
// rounds to nearest even); 24-bit sign-extended, times 2^-23
__device__ __forceinline__ float rs_sample(const uint8_t* p, int width) {
  switch (width) {
    case 1: return ((float)p[0] - 128.0f) / 128.0f;
    case 2: return (float)(int16_t)(uint16_t)(p[0] | (p[1] << 8)) * 0x1p-15f;
    case 3: {
      int32_t v = p[0] | (p[1] << 8) | (p[2] << 16);
      v = v >= (1 << 23) ? v - (1 << 24) : v;
      return (float)v * 0x1p-23f;
    }
    default: return (float)(int32_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24)) * 0x1p-31f;
  }
}

// mono frame: numpy's mean(axis=1, dtype=float32) over the channels -- its fp32 sum (in channel order below 8 channels; 8 channels
// go through its 8-accumulator block, a balanced tree) and one IEEE division by the count
__device__ __forceinline__ float rs_frame(const uint8_t* p, int width, int channels) {
  if (channels == 1) return rs_sample(p, width);
  float s;
  if (channels == 8) {
    float r[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) r[c] = rs_sample(p + c * width, width);
    s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  } else {
    s = rs_sample(p, width);
    for (int c = 1; c < channels; ++c) s += rs_sample(p + c * width, width);
  }
  return __fdiv_rn(s, (float)channels);
}

// P == Q: wave[b, t] = frame t of the row for t < min(n_orig, n_calc), 0 behind
__global__ __launch_bounds__(RS_BLOCK) void wave_decode_kernel(ResampleArgs a) {
  const int b = blockIdx.y;
  const int t0 = blockIdx.x * RS_TILE;
  const int tile = min(RS_TILE, a.L - t0);
  const int fb = a.width * a.channels;
  const int n_orig = max(0, (int)min<int64_t>(a.rows[2 * b], a.row_bytes / fb));
  const int n = min(n_orig, a.rows[2 * b + 1]);
  const uint8_t* row = a.pcm + (int64_t)b * a.row_bytes;
  float* out = a.wave + (int64_t)b * a.L + t0;
  for (int o = threadIdx.x; o < tile; o += RS_BLOCK)
    out[o] = t0 + o < n ? rs_frame(row + (int64_t)(t0 + o) * fb, a.width, a.channels) : 0.f;
}

template <bool UNI>
__global__ __launch_bounds__(RS_BLOCK) void wave_resample_kernel(ResampleArgs a) {
  extern __shared__ float rs_x[];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int t0 = blockIdx.x * RS_TILE;
  const int tile = min(RS_TILE, a.L - t0);                       // outputs of this workgroup (the grid covers L exactly)
  const int fb = a.width * a.channels;
  const int n_orig = max(0, (int)min<int64_t>(a.rows[2 * b], a.row_bytes / fb));   // never a byte outside the row
  const int n_calc = max(0, min(a.rows[2 * b + 1], a.L));
  float* out = a.wave + (int64_t)b * a.L + t0;
  const int live = min(tile, n_calc - t0);                       // outputs below n_calc; <= 0: the tile is all zeros
  if (live <= 0) {
    for (int o = tid; o < tile; o += RS_BLOCK) out[o] = 0.f;
    return;
  }
  const int K = a.n_left + a.n_right;
  const int64_t first = (int64_t)t0 * a.P / a.Q - (a.n_left - 1);
  const int span = (int)((int64_t)(t0 + live - 1) * a.P / a.Q - (a.n_left - 1) + K - first);   // <= the host's bound
  const uint8_t* row = a.pcm + (int64_t)b * a.row_bytes;
  for (int u = tid; u < span; u += RS_BLOCK) {
    const int64_t j = first + u;
    const float v = (j >= 0 && j < n_orig) ? rs_frame(row + j * fb, a.width, a.channels) : 0.f;
    if (UNI) rs_x[(u % a.P) * a.plane + u / a.P] = v;
    else rs_x[u] = v;
  }
  float* gs = rs_x + a.plane * a.P;                              // UNI: the K taps in signal order, behind the planes
  if (UNI)
    for (int m = tid; m < K; m += RS_BLOCK) gs[m] = a.taps[m < a.n_left ? a.n_left - 1 - m : m];
  __syncthreads();
  if (UNI) {
    float acc[RS_PER];
#pragma unroll
    for (int r = 0; r < RS_PER; ++r) acc[r] = 0.f;
    int pl = 0, slot = 0;                                        // plane and slot of tap m: m % P, m / P
#pragma unroll 4
    for (int m = 0; m < K; ++m) {
      const float g = gs[m];                                     // one address for the whole wave: an LDS broadcast
      const float* x = rs_x + pl * a.plane + slot + tid;
#pragma unroll
      for (int r = 0; r < RS_PER; ++r) acc[r] = fmaf(g, x[r * RS_BLOCK], acc[r]);   // (slots past `span` are never stored)
      if (++pl == a.P) {
        pl = 0;
        ++slot;
      }
    }
#pragma unroll
    for (int r = 0; r < RS_PER; ++r) {
      const int o = tid + r * RS_BLOCK;
      if (o < tile) out[o] = o < live ? acc[r] : 0.f;
    }
  } else {
    for (int o = tid; o < tile; o += RS_BLOCK) {
      float acc = 0.f;
      if (o < live) {
        const int64_t tp = (int64_t)(t0 + o) * a.P;
        const int64_t nn = tp / a.Q;
        const float* g = a.taps + (tp - nn * a.Q) * K;
        const float* x = rs_x + (nn - (a.n_left - 1) - first);
        for (int m = 0; m < a.n_left; ++m) acc = fmaf(g[a.n_left - 1 - m], x[m], acc);
        for (int m = a.n_left; m < K; ++m) acc = fmaf(g[m], x[m], acc);
      }
      out[o] = acc;
    }
  }
}

}  // namespace

extern "C" int taco_wave_resample(const uint8_t* pcm, int64_t row_bytes, int width, int channels, const int32_t* rows,
                                  const float* taps, int P, int Q, int n_left, int n_right, float* wave, int B, int L,
                                  void* stream) {
  TACO_REQUIRE(pcm && rows && wave, "wave_resample: null pointer");
  TACO_REQUIRE(width >= 1 && width <= 4 && channels >= 1 && channels <= 8, "wave_resample: width=%d outside 1..4 or channels=%d outside 1..8",
               width, channels);
  TACO_REQUIRE(P >= 1 && Q >= 1 && n_left >= 1 && n_right >= 1, "wave_resample: P=%d Q=%d n_left=%d n_right=%d must all be >= 1", P, Q,
               n_left, n_right);
  TACO_REQUIRE(taps || P == Q, "wave_resample: taps is NULL and P=%d != Q=%d", P, Q);
  TACO_REQUIRE(B > 0 && B <= 65535 && L > 0, "wave_resample: B=%d (1..65535) L=%d", B, L);
  TACO_REQUIRE(row_bytes > 0 && row_bytes % (width * channels) == 0, "wave_resample: row_bytes=%lld is not a positive multiple of width * channels = %d",
               (long long)row_bytes, width * channels);
  ResampleArgs a;
  a.pcm = pcm;
  a.rows = rows;
  a.taps = taps;
  a.wave = wave;
  a.row_bytes = row_bytes;
  a.width = width;
  a.channels = channels;
  a.P = P;
  a.Q = Q;
  a.n_left = n_left;
  a.n_right = n_right;
  a.L = L;
  a.plane = 0;
  const dim3 grid((unsigned)cdiv(L, RS_TILE), (unsigned)B);
  hipStream_t s = as_stream(stream);
  if (P == Q) {
    TACO_KLAUNCH(wave_decode_kernel, grid, dim3(RS_BLOCK), 0, s, a);   // decode-only: no filter, taps is not read
  } else {
    // frames a tile reads: the positions of its first and last output are at most (RS_TILE - 1) P / Q + 1 apart
    const int64_t span = (int64_t)(RS_TILE - 1) * P / Q + 1 + n_left + n_right;
    int64_t lds = span * 4;
    if (Q == 1) {
      a.plane = (int)((span + P - 1) / P);   // last slot stored (span - 1) / P; last slot read RS_TILE - 1 + (K - 1) / P, not behind it
      lds = ((int64_t)a.plane * P + n_left + n_right) * 4;   // and the taps in signal order behind the planes
    }
    TACO_REQUIRE(lds <= RS_LDS_MAX, "wave_resample: P=%d Q=%d with %d taps needs %lld bytes of LDS per tile, more than %lld", P, Q,
                 n_left + n_right, (long long)lds, (long long)RS_LDS_MAX);
    if (Q == 1) TACO_KLAUNCH(wave_resample_kernel<true>, grid, dim3(RS_BLOCK), (size_t)lds, s, a);
    else TACO_KLAUNCH(wave_resample_kernel<false>, grid, dim3(RS_BLOCK), (size_t)lds, s, a);
  }
  TACO_LAUNCH_CHECK("wave_resample");
  return TACO_OK;
}
