// frames.hip -- the synthesis frame chain: what happens to the decoder's output between the model and the vocoder, and the pitch
// read-outs over the same magnitude frames (include/taco_hip.h taco_denorm_unframe, taco_frames_stretch, taco_frames_stretch_curve,
// taco_frames_pitch, taco_frames_pitch_curve, taco_frames_sharpen, taco_frames_formant, taco_frames_cepstats, taco_frames_f0,
// taco_f0_stats, taco_path_f0_scores).  Every entry point stands behind its kernels with the refusals that guard them; each kernel's
// comment has its form and why.  The cosine products of frames_pitch_kernel, frames_sharpen_kernel,
// frames_formant_kernel, frames_cepstats_kernel and frames_f0_kernel are fp32 MFMAs; everything else here is bound by memory.
#include <type_traits>

#include "common.h"
#include "frames.h"
#include "kernels.h"

namespace {

// Inverse r-frame layout + de-normalisation (audio.reshape_frames(forward=False), audio.py:29-35; test.py:64
// `out * stft_std + stft_mean`).  out (B, Td, r*C): row 4c + j, column i*C + ch holds frame 4rc + 4i + j, feature ch.
// spec (B, F, C) (nullable) = chronological log-magnitude frames, F = (Td / 4) * 4 * r (only whole chunks, like the
// reference); mag_t (B, C, F) (nullable) = exp(spec) transposed = the (1 + n_fft/2, frames) magnitude matrix
// audio.invert_spectrogram hands to Griffin-Lim.  32 x 32 tiles through LDS so both images are written coalesced.
__global__ void denorm_unframe_kernel(const float* __restrict__ out, const float* __restrict__ mean,
                                      const float* __restrict__ stdv, float* __restrict__ spec, float* __restrict__ mag_t,
                                      int Td, int r, int C, int F) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z, c0 = blockIdx.x * 32, f0 = blockIdx.y * 32;
  const int RC = r * C;
  for (int j = threadIdx.y; j < 32; j += 8) {
    const int f = f0 + j, ch = c0 + threadIdx.x;
    float v = 0.f;
    if (f < F && ch < C) {
      const int chunk = f / (4 * r), rem = f - chunk * 4 * r;
      const int i = rem >> 2, jj = rem & 3;
      const int col = i * C + ch;
      v = out[((int64_t)b * Td + chunk * 4 + jj) * RC + col] * stdv[col] + mean[col];
      if (spec) spec[((int64_t)b * F + f) * C + ch] = v;
    }
    tile[j][threadIdx.x] = v;
  }
  if (!mag_t) return;
  __syncthreads();
  for (int j = threadIdx.y; j < 32; j += 8) {
    const int ch = c0 + j, f = f0 + threadIdx.x;
    if (ch < C && f < F) mag_t[((int64_t)b * C + ch) * F + f] = expf(tile[threadIdx.x][j]);
  }
}

// taco_frames_stretch: speaking rate at synthesis.  Row b of mag_t (B, C, F) is resampled along its contiguous frame axis into
// out (B, C, Fo): output frame j sits at source position p = j * s_b in units of 2^-16 frames, i = p >> 16, w = (p & 0xFFFF) 2^-16,
// and is a + (w * (c - a)) of the two frames around it -- three separately rounded fp32 operations (the pragma in the kernel's body
// keeps hipcc from contracting them; __fmul_rn / __fadd_rn are plain operators in this toolchain, see dtw.hip) -- or frame i itself,
// bit for bit and without touching frame i + 1, when w == 0.  A gather along the contiguous axis, bound by memory: lanes run
// along j, so the stores of a wave are one contiguous run and the two loads of neighbouring lanes fall into the same or adjacent
// lines.  A workgroup (64 x 4 threads) owns one row, kStretchBins bins and kStretchSpan output frames; a thread forms the index
// and weight of its four frames j0 + lane + 64 u once and walks the tile's bins with them, so every load and every store of a wave
// covers 64 consecutive output frames: 256 contiguous bytes stored, for any Fo and any alignment.  F_b, s_b and Fo_b are the same for
// the whole workgroup and read once.  A span behind Fo_b writes zeros and loads nothing.
// There is ONE form.  Two with 16-byte stores were measured beside it at 32 x 1025 x 360 and deleted (DESIGN.md 4b,
// profiles/frames_stretch_store_forms.txt): a thread owning frames j0 + 4 lane .. + 3 spreads each load of a wave over 1 KiB and
// was up to 2 x slower; this form's values turned through LDS into one 16-byte store per thread was equal within the spread.  The
// source span is not staged in LDS: that variant was not built.
//
// taco_frames_stretch_curve (a rate that varies along the utterance) is the same gather behind another time map: MAP = true reads
// the packed position (i << 16) | wq of output frame j from the map frames_stretch_map_kernel (below) left in `step_q` (B, Fo) and
// Fo_b from frames_out, instead of forming j * s_b; everything from the index and the weight on is the one body.
constexpr int kStretchBins = 16;
constexpr int kStretchSpan = 256;
template <bool MAP>
__global__ __launch_bounds__(256) void frames_stretch_kernel(const float* __restrict__ mag_t, const int32_t* __restrict__ frames,
                                                             int frames_per_unit, const int32_t* __restrict__ step_q,
                                                             float* __restrict__ out, int32_t* __restrict__ frames_out, int C, int F,
                                                             int Fo, int nspan, int ntile) {
#pragma clang fp contract(off)
  const uint32_t x = blockIdx.x;
  const int span = (int)(x % (uint32_t)nspan);
  const uint32_t t = x / (uint32_t)nspan;
  const int tile = (int)(t % (uint32_t)ntile), b = (int)(t / (uint32_t)ntile);
  int Fb = F, s = TACO_STRETCH_ONE;
  int Fob = 0;
  if constexpr (MAP) {   // the map kernel, earlier on the stream, wrote Fo_b and the positions: frames is not read again
    Fob = frames_out[b];
    Fob = Fob < 0 ? 0 : (Fob > Fo ? Fo : Fob);
    Fob = __builtin_amdgcn_readfirstlane(Fob);
  } else {
    Fb = row_frames(frames, frames_per_unit, b, F);
    if (step_q) {
      s = step_q[b];
      s = s < TACO_STRETCH_MIN_STEP ? TACO_STRETCH_MIN_STEP : (s > TACO_STRETCH_MAX_STEP ? TACO_STRETCH_MAX_STEP : s);
    }
    if (Fb > 0) {
      const uint32_t need = ((uint32_t)(Fb - 1) << 16) / (uint32_t)s + 1u;   // (Fb <= 8192: the shift stays below 2^29)
      Fob = need > (uint32_t)Fo ? Fo : (int)need;
    }
    Fb = __builtin_amdgcn_readfirstlane(Fb);
    s = __builtin_amdgcn_readfirstlane(s);
    Fob = __builtin_amdgcn_readfirstlane(Fob);
    if (span == 0 && tile == 0 && threadIdx.x == 0 && threadIdx.y == 0) frames_out[b] = Fob;
  }

  const int j0 = span * kStretchSpan, lane = threadIdx.x;
  const int k0 = tile * kStretchBins;
  int jj[4], i0[4], i1[4];
  float w[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    jj[u] = j0 + lane + 64 * u;
    // j < Fo_b: p <= (F_b - 1) << 16, so i <= F_b - 1, and i == F_b - 1 only with w == 0 -- i1 then stays i.  j >= Fo_b: frame 0 is
    // named and nothing is loaded (j < 8192 and s <= 2^18: the product fits 32 bits either way)
    uint32_t p;
    if constexpr (MAP) p = jj[u] < Fob ? (uint32_t)step_q[(int64_t)b * Fo + jj[u]] : 0u;   // (>= 0 below Fo_b: i < 8192)
    else p = jj[u] < Fob ? (uint32_t)jj[u] * (uint32_t)s : 0u;
    const uint32_t frac = p & 0xFFFFu;
    i0[u] = (int)(p >> 16);
    i1[u] = i0[u] + (frac != 0u ? 1 : 0);
    if constexpr (MAP) i0[u] = min(i0[u], F - 1), i1[u] = min(i1[u], F - 1);   // (the map names frames below F_b; the bounds do not rest on it)
    w[u] = (float)frac * (1.0f / 65536.0f);   // exact: 16 bits times a power of two
  }
  const bool live = j0 < Fob;   // (uniform over the workgroup)
  for (int kk = threadIdx.y; kk < kStretchBins; kk += 4) {
    const int k = k0 + kk;
    if (k >= C) break;
    const float* __restrict__ src = mag_t + ((int64_t)b * C + k) * F;
    float* __restrict__ dst = out + ((int64_t)b * C + k) * Fo;
    float y[4] = {0.f, 0.f, 0.f, 0.f};
    if (live) {
      float a[4], c[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {   // all loads first
        if (jj[u] < Fob) {
          a[u] = src[i0[u]];
          c[u] = src[i1[u]];
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (jj[u] < Fob) {
          const float d = c[u] - a[u];
          const float m = w[u] * d;
          y[u] = i1[u] != i0[u] ? a[u] + m : a[u];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (jj[u] < Fo) dst[jj[u]] = y[u];
  }
}

// The time map of taco_frames_stretch_curve: source frame i of row b lasts d_i = clamp(dur_q[b, i]) output frames in units of 2^-16,
// D_i = d_0 + .. + d_{i-1} is where it starts, and output frame j sits in the source frame i with D_i <= j << 16 < D_{i+1}, at the
// fraction wq = ((q - D_i) << 16) / d_i of it (include/taco_hip.h has the definition).  All integers: D reaches 2^31 at F = 8192 and
// d = 2^18, so it is unsigned.  One workgroup of 1024 threads per row: a thread sums its ceil(F_b / 1024) <= 8 consecutive durations,
// the 1024 sums are scanned in LDS, the thread writes its D_i (32 KB at F = 8192); then a thread per output frame finds i by binary
// search in LDS -- 13 probes -- and does the one 64-bit division.  B workgroups on 256 CUs is no way to fill the chip; the call is a
// few microseconds in front of a gather that is bound by memory, and the map is an output the timings need anyway.
constexpr int kMapThreads = 1024;
__device__ __forceinline__ uint32_t stretch_dur(const int32_t* __restrict__ dq, int i) {
  int d = dq ? dq[i] : TACO_STRETCH_ONE;
  d = d < TACO_STRETCH_MIN_STEP ? TACO_STRETCH_MIN_STEP : (d > TACO_STRETCH_MAX_STEP ? TACO_STRETCH_MAX_STEP : d);
  return (uint32_t)d;
}
__global__ __launch_bounds__(kMapThreads) void frames_stretch_map_kernel(const int32_t* __restrict__ frames, int frames_per_unit,
                                                                         const int32_t* __restrict__ dur_q,
                                                                         int32_t* __restrict__ frames_out, int32_t* __restrict__ src, int F,
                                                                         int Fo) {
  __shared__ uint32_t D[TACO_STRETCH_MAX_FRAMES];
  __shared__ uint32_t part[kMapThreads];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Fb = row_frames_uniform(frames, frames_per_unit, b, F);
  src += (int64_t)b * Fo;
  if (Fb == 0) {   // (uniform)
    for (int j = tid; j < Fo; j += kMapThreads) src[j] = -1;
    if (tid == 0) frames_out[b] = 0;
    return;
  }
  const int32_t* __restrict__ dq = dur_q ? dur_q + (int64_t)b * F : nullptr;   // (columns behind F_b are never read)
  const int per = (Fb + kMapThreads - 1) / kMapThreads, i0 = tid * per;
  uint32_t sum = 0;
  for (int u = 0; u < per; ++u)
    if (i0 + u < Fb) sum += stretch_dur(dq, i0 + u);
  part[tid] = sum;
  __syncthreads();
  for (int off = 1; off < kMapThreads; off <<= 1) {   // inclusive scan of the threads' sums (at most 2^31 in all: no wrap)
    const uint32_t v = tid >= off ? part[tid - off] : 0u;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  uint32_t run = part[tid] - sum;
  for (int u = 0; u < per; ++u)
    if (i0 + u < Fb) {
      D[i0 + u] = run;
      run += stretch_dur(dq, i0 + u);
    }
  __syncthreads();
  const uint32_t need = (D[Fb - 1] >> 16) + 1u;
  const int Fob = need > (uint32_t)Fo ? Fo : (int)need;
  if (tid == 0) frames_out[b] = Fob;
  for (int j = tid; j < Fo; j += kMapThreads) {
    int v = -1;
    if (j < Fob) {
      const uint32_t q = (uint32_t)j << 16;   // (j < 8192) q <= D[F_b - 1]: the search ends on F_b - 1 only with q == D there
      int lo = 0, hi = Fb - 1;
      while (lo < hi) {   // the largest i with D[i] <= q; D[0] = 0 and D rises strictly
        const int mid = (lo + hi + 1) >> 1;
        if (D[mid] <= q) lo = mid;
        else hi = mid - 1;
      }
      const uint32_t wq = (uint32_t)(((uint64_t)(q - D[lo]) << 16) / stretch_dur(dq, lo));   // (q - D_i < d_i: wq < 65536)
      v = (lo << 16) | (int)(wq & 0xFFFFu);
    }
    src[j] = v;
  }
}

// taco_frames_pitch: pitch at synthesis.  A frame's log-magnitudes L[k] are split into a log-envelope E (the cepstrum of the even
// extension, quefrencies 0 .. Q kept) and a log-excitation R = L - E; R alone is warped along the bin axis by s_b (2^-16 source bins
// per output bin) and put back under the unmoved envelope: out = exp(E[k] + R'[k]) (include/taco_hip.h has the definition).
// A workgroup of kPitchWaves waves owns kPitchFrames = 32 consecutive frames of one row: the frame index is the lane's low five
// bits, which is both the contiguous axis of mag_t / out (a half-wave reads or writes 128 contiguous bytes of one bin row) and the
// column index of a 32x32x2 fp32 MFMA.  The two cosine products are those MFMAs -- an ordered fmaf chain per element, so the bits
// of a frame do not depend on its column:
//   cepstrum  c[n][f] = sum_k cos(2 pi n k / N) (wt_k L[k][f] / N), n = 1 .. 32 NB: rows = n, the bin pairs (k, k + 1) dealt to the
//             waves round robin, the waves' partial tiles summed through LDS in wave order; c[0] is a plain sum beside it;
//   envelope  E[k][f] = c[0][f] + sum_n cos(2 pi n k / N) (2 c[n][f]): rows = 32 bins, 16 NB MFMAs per tile, the tiles dealt to the
//             waves; c[n] behind the lifter are zeros; the top bin C - 1 (cos = (-1)^n) is a sum on the side.
// NB = 1 for Q <= 32 (16 waves), 2 above (8 waves: 149 registers); which of the two runs depends on Q alone, so the bits do too.
// E stays in LDS for the frame tile (C x 32 floats, 131 KB at C = 1025; the cepstrum partials use the same bytes before it) next to
// the cosine table (N floats, indexed (n k) & (N - 1)) and the cepstra: 148 KB, one workgroup per CU.  L is NOT kept: the warp re-reads
// its two source bins (from L2 or the Infinity Cache) and takes their logarithms again -- 3 reads per element where 1 is
// compulsory, which is what keeps the kernel at four times the copy's time (profiles/frames_pitch_forms.txt, DESIGN.md 4b: the forms
// measured, and the 16-frame tile with L and E both in LDS that was not built).  With one workgroup per CU nothing hides a load but
// the workgroup's own waves, so every loop issues a batch of loads in front of the arithmetic that uses them.  Rows with
// s_b == TACO_PITCH_ONE are copied and tiles behind F_b zeroed without any of this.
constexpr int kPitchFrames = 32;
constexpr int kPitchMaxC = 1025;
constexpr int kPitchBatch = 8;         // bins a thread has in flight in the copy and in the warp

// ---- what the kernels over tiles of 32 frames share (pitch, sharpen, cepstats, F0) ----
// Where a thread stands: row b with its F_b frames, tile f0 .. f0 + 31, this lane's frame f = f0 + fl (fl: the lane's low five
// bits, h: its half of the wave), `live` in front of F_b, `inside` in front of F.  b, Fb, f0 and wave are uniform.
struct FrameTile {
  int b, Fb, f0, f, fl, h, wave;
  bool live, inside;
};
__device__ __forceinline__ FrameTile frame_tile(const int32_t* __restrict__ frames, int frames_per_unit, int F, int ntile) {
  FrameTile t;
  const int tile = (int)(blockIdx.x % (uint32_t)ntile), lane = threadIdx.x & 63;
  t.b = (int)(blockIdx.x / (uint32_t)ntile);
  t.Fb = row_frames_uniform(frames, frames_per_unit, t.b, F);
  t.fl = lane & 31, t.h = lane >> 5;
  t.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  t.f0 = tile * kPitchFrames, t.f = t.f0 + t.fl;
  t.live = t.f < t.Fb, t.inside = t.f < F;
  return t;
}

// tab[j] = cos(2 pi j / N), j < N, by the nthreads threads of the workgroup; the caller synchronises
__device__ __forceinline__ void fill_cos_table(float* tab, int N, int nthreads) {
  for (int j = threadIdx.x; j < N; j += nthreads) tab[j] = cospif((float)(2 * j) / (float)N);   // (2 j / N is exact)
}

// Nothing to compute for this tile: zeros behind the row's end, the row's own bits in front of it (kPitchBatch loads in flight per
// thread).  src and dst point at this lane's frame of bin 0.
template <int kWaves>
__device__ __forceinline__ void copy_tile(const float* __restrict__ src, float* __restrict__ dst, const FrameTile& t, int C, int F) {
  for (int kb = 2 * t.wave + t.h; kb < C; kb += 2 * kWaves * kPitchBatch) {
    float m[kPitchBatch];
#pragma unroll
    for (int u = 0; u < kPitchBatch; ++u) {
      const int k = kb + 2 * kWaves * u;
      m[u] = (t.live && k < C) ? src[k * F] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kPitchBatch; ++u) {
      const int k = kb + 2 * kWaves * u;
      if (t.inside && k < C) dst[k * F] = m[u];
    }
  }
}

// The cepstrum stage: c[n][f], n = 0 .. 32 NB, of the 32 frames of a tile into cep[n * 32 + f], rows behind the rectangular lifter
// Q zeroed.  The bin pairs (k, k + 1) are dealt to the kWaves waves round robin, each an ordered chain of 32x32x2 fp32 MFMAs, and the
// waves' partial tiles are folded through LDS in wave order; c[0] is a plain sum beside it.  This is the ONE text of these chains:
// "the same fp32 cepstra" in the pitch, sharpen and cepstats kernels means this function.  `part` is scratch of
// (kWaves 32 NB + 2 kWaves) x 32 floats.  Called by every thread of the workgroup (it has barriers); tab is filled and synchronised
// by the caller.  Behind it cep is complete and visible, and nothing reads part any more.
template <int NB, int kWaves>
__device__ __forceinline__ void cepstrum_tile(const float* __restrict__ src, bool live, int Q, int C, int F, const float* tab,
                                              float* cep, float* part) {
  constexpr int NR = 32 * NB;
  const int tid = threadIdx.x, lane = tid & 63, fl = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int N = 2 * (C - 1), mask = N - 1;
  const float wt = 2.0f / (float)N;   // (a power of two: the weight and the 1 / N cost no rounding)
  f32x16 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;
  float c0p = 0.f;
  float m[4], nx[4];   // four bin pairs per trip, the next trip's loads issued in front of this trip's arithmetic
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int k = 2 * wave + 2 * kWaves * u + h;
    m[u] = (live && k < C) ? src[k * F] : 1.0f;
  }
  for (int k0 = 2 * wave; k0 < C; k0 += 8 * kWaves) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = k0 + 8 * kWaves + 2 * kWaves * u + h;
      nx[u] = (live && k < C) ? src[k * F] : 1.0f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = k0 + 2 * kWaves * u + h;   // (k >= C: m = 1, v = 0, and the table is read at some valid index)
      const float v = logf(fmaxf(m[u], TACO_PITCH_FLOOR)) * ((k == 0 || k == C - 1) ? 0.5f * wt : wt);
      c0p += v;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
        acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(tab[((32 * nb + 1 + fl) * k) & mask], v, acc[nb], 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) m[u] = nx[u];
  }
  float* part0 = part + kWaves * NR * kPitchFrames;   // part: [wave][n - 1][f]; part0: [wave][h][f] for c[0]
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      part[((wave * NR) + 32 * nb + (r & 3) + 8 * (r >> 2) + 4 * h) * kPitchFrames + fl] = acc[nb][r];
  part0[(2 * wave + h) * kPitchFrames + fl] = c0p;
  __syncthreads();
  for (int e = tid; e < NR * kPitchFrames; e += 64 * kWaves) {   // e = (n - 1) * 32 + f
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) t += part[w * NR * kPitchFrames + e];
    cep[kPitchFrames + e] = (e >> 5) < Q ? t : 0.f;   // the rectangular lifter
  }
  if (tid < kPitchFrames) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < 2 * kWaves; ++w) t += part0[w * kPitchFrames + tid];
    cep[tid] = t;
  }
  __syncthreads();
}

// The cosine synthesis stage: X[k][f] = init[f] + sum_n cos(2 pi n k / N) (scale c[n][f]) over n = first .. last of the tile's cepstra
// into X[k * 32 + f].  Bins k < C - 1 in blocks of 32 dealt to the waves, 16 NB MFMAs per block in ascending (nb, j) with rows outside
// first .. last zero in the B operands; the top bin C - 1 (cos = (-1)^n) is a sum on the side in ascending n.  init is this lane's
// frame's start value.  Called by every thread of the workgroup; behind it X is complete and visible.
template <int NB, int kWaves>
__device__ __forceinline__ void cosine_tile(const float* tab, const float* cep, float init, float scale, int first, int last, int C,
                                            float* X) {
  const int tid = threadIdx.x, lane = tid & 63, fl = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int mask = 2 * (C - 1) - 1;
  float cb[NB][16];   // scale c[n][f], n = 32 nb + 1 + 2 j + h: this lane's B operands
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int n = 32 * nb + 1 + 2 * j + h;
      cb[nb][j] = (n >= first && n <= last) ? scale * cep[n * kPitchFrames + fl] : 0.f;
    }
  if (tid < kPitchFrames) {   // bin C - 1: cos(pi n) = (-1)^n
    float t = init;
    for (int n = first; n <= last; ++n) {
      const float c2 = scale * cep[n * kPitchFrames + tid];
      t += (n & 1) ? -c2 : c2;
    }
    X[(C - 1) * kPitchFrames + tid] = t;
  }
  const int nblk = (C - 1 + 31) >> 5;
  for (int kb = wave; kb < nblk; kb += kWaves) {
    const int k = 32 * kb + fl;
    f32x16 d;
#pragma unroll
    for (int r = 0; r < 16; ++r) d[r] = init;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int j = 0; j < 16; ++j)
        d = __builtin_amdgcn_mfma_f32_32x32x2f32(tab[((32 * nb + 1 + 2 * j + h) * k) & mask], cb[nb][j], d, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int kk = 32 * kb + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (kk < C - 1) X[kk * kPitchFrames + fl] = d[r];
    }
  }
  __syncthreads();
}

// taco_frames_pitch_curve (a pitch contour) is CURVE = true: step_q is (B, F) and the step belongs to the frame, that is to the lane
// (its low five bits), so s is a per-lane register from here on and costs no LDS.  The cepstrum and the envelope do not know s; the
// warp's k * s >> 16 takes it per lane.  The copy branch is taken when all 32 frames of the tile are at ONE or behind F_b -- every
// wave holds the same 32 frames in both halves, so one ballot per wave gives every wave the same answer -- and a ONE lane of a mixed
// tile stores its source value, no log / exp round trip.
template <int NB, int kPitchWaves, bool CURVE>
__global__ __launch_bounds__(64 * kPitchWaves) void frames_pitch_kernel(const float* __restrict__ mag_t, const int32_t* __restrict__ frames,
                                                                         int frames_per_unit, const int32_t* __restrict__ step_q, int Q,
                                                                         float* __restrict__ out, int C, int F, int ntile) {
  constexpr int NR = 32 * NB;                                // cepstrum rows n = 1 .. NR
  __shared__ float tab[2 * (kPitchMaxC - 1)];
  __shared__ float cep[(NR + 1) * kPitchFrames];             // c[n][f], n = 0 .. NR
  __shared__ float env[kPitchMaxC * kPitchFrames];           // E[k][f]; before that the waves' partial cepstra
  const FrameTile t = frame_tile(frames, frames_per_unit, F, ntile);
  const int b = t.b, f = t.f, fl = t.fl, h = t.h, wave = t.wave;
  const bool live = t.live, inside = t.inside;
  int s = TACO_PITCH_ONE;
  if constexpr (!CURVE) {
    if (step_q) {
      s = step_q[b];
      s = s < TACO_PITCH_MIN_STEP ? TACO_PITCH_MIN_STEP : (s > TACO_PITCH_MAX_STEP ? TACO_PITCH_MAX_STEP : s);
    }
    s = __builtin_amdgcn_readfirstlane(s);
  }
  const float* __restrict__ src = mag_t + (int64_t)b * C * F + f;    // (C F <= 1025 * 8192: the offsets below fit 32 bits)
  float* __restrict__ dst = out + (int64_t)b * C * F + f;
  bool plain;
  if constexpr (CURVE) {
    if (step_q && live) {   // (a frame behind F_b keeps ONE: its step is never read)
      s = step_q[(int64_t)b * F + f];
      s = s < TACO_PITCH_MIN_STEP ? TACO_PITCH_MIN_STEP : (s > TACO_PITCH_MAX_STEP ? TACO_PITCH_MAX_STEP : s);
    }
    plain = __ballot(live && s != TACO_PITCH_ONE) == 0;
  } else {
    plain = t.f0 >= t.Fb || s == TACO_PITCH_ONE;
  }
  if (plain) {   // (uniform) nothing to shift
    copy_tile<kPitchWaves>(src, dst, t, C, F);
    return;
  }
  fill_cos_table(tab, 2 * (C - 1), 64 * kPitchWaves);
  __syncthreads();
  cepstrum_tile<NB, kPitchWaves>(src, live, Q, C, F, tab, cep, env);   // (the partials in env's bytes: nothing reads them behind it)
  cosine_tile<NB, kPitchWaves>(tab, cep, cep[fl], 2.0f, 1, NR, C, env);   // the envelope: c[0] + sum of 2 c[n], zeros behind the lifter

  // ---- warp of the excitation, output ----  kPitchBatch bins per trip: every load of the trip first, at indices clamped into the
  // frame (a value from a clamped index is never used)
  for (int kb = 2 * wave + h; kb < C; kb += 2 * kPitchWaves * kPitchBatch) {
    float m0[kPitchBatch], m1[kPitchBatch];
    if (live) {
#pragma unroll
      for (int u = 0; u < kPitchBatch; ++u) {
        const int k = min(kb + 2 * kPitchWaves * u, C - 1);
        const int i = (int)(((uint32_t)k * (uint32_t)s) >> 16);   // (k s <= 1024 * 2^17)
        m0[u] = src[min(i, C - 1) * F];
        m1[u] = src[min(i + 1, C - 1) * F];
      }
    }
#pragma unroll
    for (int u = 0; u < kPitchBatch; ++u) {
      const int k = kb + 2 * kPitchWaves * u;
      if (k >= C) break;
      float y = 0.f;
      if (live) {
        const uint32_t p = (uint32_t)k * (uint32_t)s;
        const int i = (int)(p >> 16), ia = min(i, C - 1), ib = min(i + 1, C - 1);
        const uint32_t frac = p & 0xFFFFu;
        const float r0 = logf(fmaxf(m0[u], TACO_PITCH_FLOOR)) - env[ia * kPitchFrames + fl];
        const float r1 = logf(fmaxf(m1[u], TACO_PITCH_FLOOR)) - env[ib * kPitchFrames + fl];
        // i < C - 1: between two bins; i == C - 1 with w == 0: the top bin itself; beyond it the envelope alone
        const float rp = i < C - 1 ? r0 + (float)frac * (1.0f / 65536.0f) * (r1 - r0) : ((i == C - 1 && frac == 0u) ? r0 : 0.f);
        y = expf(env[k * kPitchFrames + fl] + rp);
        if constexpr (CURVE)
          if (s == TACO_PITCH_ONE) y = m0[u];   // (k s >> 16 == k: m0 is the frame's own bin) a ONE frame among shifted ones
      }
      if (inside) dst[k * F] = y;
    }
  }
}

// taco_frames_sharpen: the cepstral post-filter (include/taco_hip.h has the definition).  The shape of frames_pitch_kernel: a
// workgroup owns 32 consecutive frames of a row, the frame is the lane's low five bits, NB = 1 (16 waves) for Q <= 32 and 2 (8 waves)
// above -- chosen by Q alone, so the bits depend on Q alone.  Three stages:
//   cepstrum  cepstrum_tile above;
//   D[k][f] = sum_{n = 2 .. Q} cos(2 pi n k / N) (2 beta c[n][f]): the envelope stage of the pitch kernel started at 0 with the rows
//             n < 2 and n > Q zeroed in the B operands; D of the tile stays in LDS (C x 32 floats);
//   output    every thread reads its bins once more, y = m exp(D) takes D's place in LDS (the thread that wrote an element is the one
//             that reads it back), the squares of m and y are summed per thread, the 2 kWaves partials of a frame folded in a fixed
//             order through the bytes of the cosine table (no longer read), g = sqrt(P0 / P1), and out = y g.
// Two reads per element where one is compulsory, one logarithm and one exponential.  beta == 0 and tiles behind F_b: the pitch
// kernel's copy branch.
template <int NB, int kWaves>
__global__ __launch_bounds__(64 * kWaves) void frames_sharpen_kernel(const float* __restrict__ mag_t, const int32_t* __restrict__ frames,
                                                                      int frames_per_unit, float beta, int Q, float* __restrict__ out,
                                                                      int C, int F, int ntile) {
  constexpr int NR = 32 * NB;
  static_assert(4 * kWaves * kPitchFrames <= 2 * (kPitchMaxC - 1), "the partial sums of P0 and P1 fit the cosine table");
  static_assert((kWaves * NR + 2 * kWaves) <= kPitchMaxC, "the cepstrum partials fit D's bytes");
  __shared__ float tab[2 * (kPitchMaxC - 1)];
  __shared__ float cep[(NR + 1) * kPitchFrames];
  __shared__ float env[kPitchMaxC * kPitchFrames];   // D[k][f], then y[k][f]; before that the waves' partial cepstra
  const FrameTile t = frame_tile(frames, frames_per_unit, F, ntile);
  const int tid = threadIdx.x, fl = t.fl, h = t.h, wave = t.wave;
  const bool live = t.live, inside = t.inside;
  const float* __restrict__ src = mag_t + (int64_t)t.b * C * F + t.f;    // (C F <= 1025 * 8192: the offsets below fit 32 bits)
  float* __restrict__ dst = out + (int64_t)t.b * C * F + t.f;
  if (t.f0 >= t.Fb || beta == 0.f) {   // (uniform)
    copy_tile<kWaves>(src, dst, t, C, F);
    return;
  }
  fill_cos_table(tab, 2 * (C - 1), 64 * kWaves);
  __syncthreads();
  cepstrum_tile<NB, kWaves>(src, live, Q, C, F, tab, cep, env);
  // D; nothing reads the cosine table behind it: tab holds the partial sums
  cosine_tile<NB, kWaves>(tab, cep, 0.f, 2.0f * beta, TACO_SHARPEN_FIRST, Q, C, env);

  // ---- y and the two energies ----  a frame behind F_b inside a live tile has m = 0: y = 0, P0 = P1 = 0, g = 1
  float p0 = 0.f, p1 = 0.f;
  for (int kb = 2 * wave + h; kb < C; kb += 2 * kWaves * kPitchBatch) {
    float m[kPitchBatch];
#pragma unroll
    for (int u = 0; u < kPitchBatch; ++u) {
      const int k = kb + 2 * kWaves * u;
      m[u] = (live && k < C) ? src[k * F] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kPitchBatch; ++u) {
      const int k = kb + 2 * kWaves * u;
      if (k >= C) break;
      const float y = m[u] * expf(env[k * kPitchFrames + fl]);
      p0 += m[u] * m[u];
      p1 += y * y;
      env[k * kPitchFrames + fl] = y;
    }
  }
  tab[(2 * wave + h) * kPitchFrames + fl] = p0;
  tab[(2 * kWaves + 2 * wave + h) * kPitchFrames + fl] = p1;
  __syncthreads();
  if (tid < kPitchFrames) {
    float P0 = 0.f, P1 = 0.f;
#pragma unroll
    for (int w = 0; w < 2 * kWaves; ++w) {
      P0 += tab[w * kPitchFrames + tid];
      P1 += tab[(2 * kWaves + w) * kPitchFrames + tid];
    }
    cep[tid] = P1 == 0.f ? 1.0f : sqrtf(P0 / P1);
  }
  __syncthreads();
  const float g = cep[fl];
  if (!inside) return;
  for (int k = 2 * wave + h; k < C; k += 2 * kWaves) dst[k * F] = live ? env[k * kPitchFrames + fl] * g : 0.f;
}

// taco_frames_formant: the dual of taco_frames_pitch -- the envelope is read at k * s_b and the excitation stays (include/taco_hip.h
// has the definition).  The shape of frames_sharpen_kernel: 32 frames of a row per workgroup, the frame in the lane's low five bits,
// NB = 1 (16 waves) for Q <= 32 and 2 (8 waves) above, chosen by Q alone.  Three stages:
//   cepstrum  cepstrum_tile above;
//   E[k][f]   the envelope call of the pitch kernel (cosine_tile, init c[0], scale 2, rows 1 .. NR), so E has the same fp32 cepstra
//             and envelope by construction; E of the tile stays in LDS (C x 32 floats);
//   output    E'[k] reads E at the bins i and i + 1 that other threads own, so y cannot take E's place element by element as in the
//             sharpen kernel, and a second C x 32 array does not fit the LDS beside E.  A thread therefore keeps the y of its own
//             bins -- at most kFormantTrips kPitchBatch = 40 | 72 of them, k = 2 wave + h + 2 kWaves j -- in registers across the fold of
//             the two energies (through the cosine table's bytes, as in the sharpen kernel) and stores y g from them: two reads per
//             element where one is compulsory, one logarithm and one exponential.  The loop over the trips has a constant trip count
//             and is unrolled, which is what keeps y in registers; trips at and behind C do nothing.  The other form -- the bins run
//             twice, once for the energies and once to store y g -- was measured beside it at 32 x 1025 x 360 | 720 and deleted: 83 |
//             126 us against 70 | 106 (profiles/frames_formant_forms.txt).
// s_b == TACO_PITCH_ONE and tiles behind F_b: the pitch kernel's copy branch.
template <int kWaves>
constexpr int kFormantTrips = (kPitchMaxC + 2 * kWaves * kPitchBatch - 1) / (2 * kWaves * kPitchBatch);
template <int NB, int kWaves>
__global__ __launch_bounds__(64 * kWaves) void frames_formant_kernel(const float* __restrict__ mag_t, const int32_t* __restrict__ frames,
                                                                      int frames_per_unit, const int32_t* __restrict__ step_q, int Q,
                                                                      float* __restrict__ out, int C, int F, int ntile) {
  constexpr int NR = 32 * NB;
  constexpr int NT = kFormantTrips<kWaves>;
  static_assert(4 * kWaves * kPitchFrames <= 2 * (kPitchMaxC - 1), "the partial sums of P0 and P1 fit the cosine table");
  static_assert((kWaves * NR + 2 * kWaves) <= kPitchMaxC, "the cepstrum partials fit E's bytes");
  __shared__ float tab[2 * (kPitchMaxC - 1)];
  __shared__ float cep[(NR + 1) * kPitchFrames];
  __shared__ float env[kPitchMaxC * kPitchFrames];   // E[k][f]; before that the waves' partial cepstra
  const FrameTile t = frame_tile(frames, frames_per_unit, F, ntile);
  const int tid = threadIdx.x, fl = t.fl, h = t.h, wave = t.wave;
  const bool live = t.live, inside = t.inside;
  int s = TACO_PITCH_ONE;
  if (step_q) {
    s = step_q[t.b];
    s = s < TACO_PITCH_MIN_STEP ? TACO_PITCH_MIN_STEP : (s > TACO_PITCH_MAX_STEP ? TACO_PITCH_MAX_STEP : s);
  }
  s = __builtin_amdgcn_readfirstlane(s);
  const float* __restrict__ src = mag_t + (int64_t)t.b * C * F + t.f;    // (C F <= 1025 * 8192: the offsets below fit 32 bits)
  float* __restrict__ dst = out + (int64_t)t.b * C * F + t.f;
  if (t.f0 >= t.Fb || s == TACO_PITCH_ONE) {   // (uniform) nothing to shift
    copy_tile<kWaves>(src, dst, t, C, F);
    return;
  }
  fill_cos_table(tab, 2 * (C - 1), 64 * kWaves);
  __syncthreads();
  cepstrum_tile<NB, kWaves>(src, live, Q, C, F, tab, cep, env);
  // the envelope; nothing reads the cosine table behind it: tab holds the partial sums
  cosine_tile<NB, kWaves>(tab, cep, cep[fl], 2.0f, 1, NR, C, env);

  // ---- y and the two energies ----  a frame behind F_b inside a live tile has m = 0: y = 0, P0 = P1 = 0, g = 1.  The envelope is
  // read at indices clamped into the frame; beyond the top bin it is held at E[C - 1]
  float y[NT * kPitchBatch];
  float p0 = 0.f, p1 = 0.f;
#pragma unroll
  for (int trip = 0; trip < NT; ++trip) {
    const int kb = 2 * wave + h + 2 * kWaves * kPitchBatch * trip;
    float m[kPitchBatch];
#pragma unroll
    for (int u = 0; u < kPitchBatch; ++u) {
      const int k = kb + 2 * kWaves * u;
      m[u] = (live && k < C) ? src[k * F] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kPitchBatch; ++u) {
      const int k = kb + 2 * kWaves * u;
      float v = 0.f;
      if (k < C) {
        const uint32_t p = (uint32_t)k * (uint32_t)s;   // (k s <= 1024 * 2^17)
        const int i = (int)(p >> 16);
        const float e0 = env[min(i, C - 1) * kPitchFrames + fl], e1 = env[min(i + 1, C - 1) * kPitchFrames + fl];
        const float ep = i < C - 1 ? e0 + (float)(p & 0xFFFFu) * (1.0f / 65536.0f) * (e1 - e0) : e0;
        v = m[u] * expf(ep - env[k * kPitchFrames + fl]);
        p0 += m[u] * m[u];
        p1 += v * v;
      }
      y[trip * kPitchBatch + u] = v;
    }
  }
  tab[(2 * wave + h) * kPitchFrames + fl] = p0;
  tab[(2 * kWaves + 2 * wave + h) * kPitchFrames + fl] = p1;
  __syncthreads();
  if (tid < kPitchFrames) {
    float P0 = 0.f, P1 = 0.f;
#pragma unroll
    for (int w = 0; w < 2 * kWaves; ++w) {
      P0 += tab[w * kPitchFrames + tid];
      P1 += tab[(2 * kWaves + w) * kPitchFrames + tid];
    }
    cep[tid] = P1 == 0.f ? 1.0f : sqrtf(P0 / P1);
  }
  __syncthreads();
  const float g = cep[fl];
  if (!inside) return;
#pragma unroll
  for (int j = 0; j < NT * kPitchBatch; ++j) {
    const int k = 2 * wave + h + 2 * kWaves * j;
    if (k < C) dst[k * F] = live ? y[j] * g : 0.f;
  }
}

// taco_frames_cepstats: per row the sums over the live frames of every cepstral coefficient and of its square.  The first launch is
// the sharpening kernel's first stage per tile of 32 frames (cepstrum_tile: the same chains, so the same fp32 cepstra), then thread n
// adds the tile's live frames of c[n] and of c[n]^2 in fp64 in frame order and leaves the pair in the workspace at [b][tile][n] --
// a tile behind F_b leaves zeros and loads nothing.  The second launch (one workgroup per row, thread n) folds the tiles in tile
// order.  No atomics; the workspace is written before it is read, so its contents on entry do not matter.  sums is written as
// 32-bit halves: it may sit at any 4-byte alignment; the workspace is aligned up to 8 bytes inside its slack.
__device__ __forceinline__ void store_f64_halves(double* p, double v) {
  uint32_t* q = reinterpret_cast<uint32_t*>(p);
  q[0] = (uint32_t)__double2loint(v);
  q[1] = (uint32_t)__double2hiint(v);
}
template <int NB, int kWaves>
__global__ __launch_bounds__(64 * kWaves) void frames_cepstats_kernel(const float* __restrict__ mag_t, const int32_t* __restrict__ frames,
                                                                       int frames_per_unit, int Q, double* __restrict__ partial, int C,
                                                                       int F, int ntile) {
  constexpr int NR = 32 * NB;
  __shared__ float tab[2 * (kPitchMaxC - 1)];
  __shared__ float cep[(NR + 1) * kPitchFrames];
  __shared__ float part[(kWaves * NR + 2 * kWaves) * kPitchFrames];
  const FrameTile t = frame_tile(frames, frames_per_unit, F, ntile);
  const int tid = threadIdx.x;
  double* __restrict__ mine = partial + (int64_t)blockIdx.x * (2 * (Q + 1));
  if (t.f0 >= t.Fb) {   // (uniform)
    if (tid <= Q) mine[2 * tid] = 0.0, mine[2 * tid + 1] = 0.0;
    return;
  }
  fill_cos_table(tab, 2 * (C - 1), 64 * kWaves);
  __syncthreads();
  cepstrum_tile<NB, kWaves>(mag_t + (int64_t)t.b * C * F + t.f, t.live, Q, C, F, tab, cep, part);
  if (tid <= Q) {
    const int nl = t.Fb - t.f0 < kPitchFrames ? t.Fb - t.f0 : kPitchFrames;
    double s = 0.0, s2 = 0.0;
    for (int j = 0; j < nl; ++j) {
      const double c = (double)cep[tid * kPitchFrames + j];
      s += c;
      s2 += c * c;   // (the square of a float is exact in fp64: contracted or not, one rounding)
    }
    mine[2 * tid] = s, mine[2 * tid + 1] = s2;
  }
}
__global__ __launch_bounds__(128) void frames_cepstats_fold_kernel(const double* __restrict__ partial, const int32_t* __restrict__ frames,
                                                                    int frames_per_unit, int Q, double* __restrict__ sums,
                                                                    int32_t* __restrict__ count, int F, int ntile) {
  static_assert(TACO_PITCH_MAX_LIFTER + 1 <= 128, "one thread per quefrency");
  const int b = blockIdx.x, n = threadIdx.x;
  if (n == 0) count[b] = row_frames(frames, frames_per_unit, b, F);
  if (n > Q) return;
  const double* __restrict__ p = partial + ((int64_t)b * ntile) * (2 * (Q + 1)) + 2 * n;
  double s = 0.0, s2 = 0.0;
  for (int t = 0; t < ntile; ++t) s += p[(int64_t)t * (2 * (Q + 1))], s2 += p[(int64_t)t * (2 * (Q + 1)) + 1];
  store_f64_halves(sums + ((int64_t)b * (Q + 1) + n) * 2, s);
  store_f64_halves(sums + ((int64_t)b * (Q + 1) + n) * 2 + 1, s2);
}

// taco_frames_f0: the pitch of a magnitude frame.  By Wiener-Khinchin the cosine transform of the power spectrum is the
// autocorrelation of the windowed frame: p[k] = u[k] weight[k] m[k]^2, r[n] = sum_k p[k] cos(2 pi n k / N) over the band of lags
// n = lag_min - 1 .. lag_max + 1, y[n] = (r[n] / r0) gain[n - lag_min + 1], and the period is the first high local maximum of y,
// refined by a parabola (include/taco_hip.h has the definition and the exact rules of the pick).
// The form of frames_pitch_kernel's cepstrum: a workgroup of kF0Waves waves owns kF0Frames = 32 consecutive frames of one row, the
// frame index is the lane's low five bits (128 contiguous bytes per bin row, and the column of a 32x32x2 fp32 MFMA).  p is formed
// once per element into LDS (C x 32 floats, and one row of zeros behind the top bin, which pairs with it), its r0 summed beside it
// from 2 kF0Waves partials in a fixed order.  The product (L x C) (C x 32) is dealt to the waves by tiles of 32 lags: wave w owns
// tiles w and, for L > 32 kF0Waves, w + kF0Waves (NT = 1 | 2; a tile's chain of MFMAs runs over the bin pairs in ascending order
// whichever NT, so the bits do not depend on it), A from the cosine table indexed (n k) & (N - 1), B from p.  Behind a barrier the
// y tile takes p's place in LDS; the pick reads it with 2 kF0Waves threads per frame, each over a contiguous run of lags -- the
// largest candidate (a maximum: no order), then the smallest lag at or above ratio * g -- and one thread per frame finishes.
// A tile behind F_b writes zeros and loads nothing; a frame behind F_b inside a live tile has p = 0, hence r0 = 0 and zeros.
constexpr int kF0Frames = 32;
static_assert(kF0Frames == kPitchFrames, "frame_tile's tile");
constexpr int kF0Waves = 8;
constexpr int kF0Parts = 2 * kF0Waves;   // threads per frame: forming p, and in the pick
static_assert(TACO_F0_MAX_LAGS <= 2 * 32 * kF0Waves, "two tiles of 32 lags per wave at the most");
template <int NT>
__global__ __launch_bounds__(64 * kF0Waves) void frames_f0_kernel(const float* __restrict__ mag_t, const int32_t* __restrict__ frames,
                                                                  int frames_per_unit, const float* __restrict__ weight,
                                                                  const float* __restrict__ gain, int lag_min, int lag_max, float ratio,
                                                                  float threshold, float* __restrict__ period,
                                                                  float* __restrict__ strength, float* __restrict__ acf, int C, int F,
                                                                  int ntile) {
#pragma clang fp contract(off)
  __shared__ float tab[2 * (kPitchMaxC - 1)];
  __shared__ float pw[(kPitchMaxC + 1) * kF0Frames];   // p[k][f], k = 0 .. C (row C: zeros); behind the product y[j][f]
  __shared__ float part[kF0Parts * kF0Frames];         // the partial sums of r0; in the pick the parts' largest candidates
  __shared__ int first[kF0Parts * kF0Frames];          // the parts' first candidates at or above ratio * g
  __shared__ float r0s[kF0Frames];
  const FrameTile t = frame_tile(frames, frames_per_unit, F, ntile);
  const int tid = threadIdx.x, b = t.b, f = t.f, fl = t.fl, h = t.h, wave = t.wave;
  const int pt = 2 * wave + h;   // = tid >> 5
  const int L = lag_max - lag_min + 3;
  const bool live = t.live, inside = t.inside;
  float* __restrict__ ac = acf ? acf + (int64_t)b * L * F + f : nullptr;   // (L F <= 512 * 8192: the offsets below fit 32 bits)
  if (t.f0 >= t.Fb) {   // (uniform) behind the row's end
    if (inside) {
      if (tid < kF0Frames) period[(int64_t)b * F + f] = strength[(int64_t)b * F + f] = 0.f;
      if (ac)
        for (int j = pt; j < L; j += kF0Parts) ac[j * F] = 0.f;
    }
    return;
  }
  const int N = 2 * (C - 1), mask = N - 1;
  fill_cos_table(tab, N, 64 * kF0Waves);   // (visible behind the barrier below)

  // ---- p and r0 ----
  const float* __restrict__ src = mag_t + (int64_t)b * C * F + f;   // (C F <= 1025 * 8192)
  float r0p = 0.f;
#pragma unroll 4
  for (int k = pt; k <= C; k += kF0Parts) {
    float v = 0.f;
    if (live && k < C) {
      const float m = src[k * F];
      const float w = weight ? weight[k] : 1.0f;
      v = (((k == 0 || k == C - 1) ? 1.0f : 2.0f) * w) * (m * m);
    }
    pw[k * kF0Frames + fl] = v;
    r0p += v;
  }
  part[pt * kF0Frames + fl] = r0p;
  __syncthreads();
  if (tid < kF0Frames) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < kF0Parts; ++w) t += part[w * kF0Frames + tid];
    r0s[tid] = t;
  }

  // ---- r[n] over the band ----
  f32x16 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  if (32 * wave < L) {   // (uniform per wave; rows at and behind L of a tile are computed at valid table indices and dropped)
    const int n0 = lag_min - 1 + 32 * wave + fl;
#pragma unroll 4
    for (int k0 = 0; k0 < C; k0 += 2) {
      const int k = k0 + h;   // (k == C: the row of zeros)
      const float v = pw[k * kF0Frames + fl];
#pragma unroll
      for (int j = 0; j < NT; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(tab[((n0 + 32 * kF0Waves * j) * k) & mask], v, acc[j], 0, 0, 0);
    }
  }
  __syncthreads();   // (nothing reads p from here on: pw is the y tile's)
  const float r0 = r0s[fl];
  const bool sounding = r0 > 0.f;   // (false for zero, underflowed and NaN)
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = 32 * (wave + kF0Waves * j) + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (row < L) pw[row * kF0Frames + fl] = sounding ? __fdiv_rn(acc[j][r], r0) * (gain ? gain[row] : 1.0f) : 0.f;
    }
  __syncthreads();
  if (ac && inside)
    for (int j = pt; j < L; j += kF0Parts) ac[j * F] = pw[j * kF0Frames + fl];

  // ---- the pick ----  row i of the tile is lag lag_min - 1 + i; the candidates are rows 1 .. L - 2
  const int chunk = (L - 2 + kF0Parts - 1) / kF0Parts;
  const int lo = 1 + pt * chunk, hi = min(lo + chunk, L - 1);
  float g = -INFINITY;
  for (int i = lo; i < hi; ++i) {
    const float y0 = pw[i * kF0Frames + fl];
    if (y0 > pw[(i - 1) * kF0Frames + fl] && y0 >= pw[(i + 1) * kF0Frames + fl] && y0 > g) g = y0;
  }
  part[pt * kF0Frames + fl] = g;   // (its sums of r0 were read in front of the product)
  __syncthreads();
  g = -INFINITY;
#pragma unroll
  for (int w = 0; w < kF0Parts; ++w) {
    const float v = part[w * kF0Frames + fl];
    g = v > g ? v : g;
  }
  const float bar = ratio * g;
  int at = 0x7fffffff;
  for (int i = lo; i < hi; ++i) {
    const float y0 = pw[i * kF0Frames + fl];
    if (y0 > pw[(i - 1) * kF0Frames + fl] && y0 >= pw[(i + 1) * kF0Frames + fl] && y0 >= bar) {
      at = i;
      break;
    }
  }
  first[pt * kF0Frames + fl] = at;
  __syncthreads();
  if (tid < kF0Frames && inside) {
#pragma unroll
    for (int w = 0; w < kF0Parts; ++w) at = min(at, first[w * kF0Frames + tid]);
    float per = 0.f, str = 0.f;
    if (g > -INFINITY && at != 0x7fffffff) {
      const float ym = pw[(at - 1) * kF0Frames + tid], y0 = pw[at * kF0Frames + tid], yp = pw[(at + 1) * kF0Frames + tid];
      if (y0 >= threshold) {
        const float a = ym - yp;
        const float t = y0 + y0;
        const float d = (ym - t) + yp;
        float delta = 0.f;
        if (d != 0.f) {
          delta = __fdiv_rn(0.5f * a, d);
          delta = delta < -0.5f ? -0.5f : (delta > 0.5f ? 0.5f : delta);
        }
        per = (float)(lag_min - 1 + at) + delta;
        str = y0;
      }
    }
    period[(int64_t)b * F + f] = per;
    strength[(int64_t)b * F + f] = str;
  }
}

// taco_f0_stats: count, mean and population standard deviation of x_f = log2(period) -- or log2(other) - log2(period), the octaves
// by which period's pitch lies above other's -- over the voiced frames of a row.  One workgroup per row, two passes (the sum, then
// the squares around the mean), a thread's frames in ascending order and the threads' partials down a fixed tree: f0_row_stats of
// frames.h, which taco_f0_range_curve (f0_curve.hip) centres its rows with.
__global__ __launch_bounds__(256) void f0_stats_kernel(const float* __restrict__ period, const float* __restrict__ other,
                                                       const int32_t* __restrict__ frames, int frames_per_unit,
                                                       float* __restrict__ stats, int F) {
  __shared__ float red[256];
  __shared__ int cnt[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Fb = row_frames(frames, frames_per_unit, b, F);
  const F0RowStats r = f0_row_stats(period + (int64_t)b * F, other ? other + (int64_t)b * F : nullptr, Fb, tid, red, cnt);
  if (tid == 0) {
    stats[3 * b] = (float)r.n;
    stats[3 * b + 1] = r.mean;
    stats[3 * b + 2] = r.n > 0 ? sqrtf(r.ss / (float)r.n) : 0.f;
  }
}

// taco_path_f0_scores: two pitch tracks compared cell by cell along a warping path (taco_frame_dtw_path's).  One workgroup per
// row; thread tid takes the cells t = tid, tid + 256, ... in ascending order (at most 8 of the 2047 a path can have), and the
// threads' five counts and two sums go down the fixed tree f0_stats_kernel uses: no atomics, the same arguments give the same
// bits.  The gross test is two single products (contraction is off in this kernel, as the header promises).
__global__ __launch_bounds__(256) void path_f0_scores_kernel(const float* __restrict__ period_a, const float* __restrict__ period_b,
                                                             const int32_t* __restrict__ path_a, const int32_t* __restrict__ path_b,
                                                             const int32_t* __restrict__ steps, float gross,
                                                             int32_t* __restrict__ counts, float* __restrict__ means, int Fa, int Fb) {
#pragma clang fp contract(off)
  __shared__ float red[2][256];
  __shared__ int cnt[5][256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int P = Fa + Fb - 1;
  int n = steps[b];
  n = n < 0 ? 0 : (n > P ? P : n);
  const float* __restrict__ ra = period_a + (int64_t)b * Fa;
  const float* __restrict__ rb = period_b + (int64_t)b * Fb;
  const int32_t* __restrict__ ia = path_a + (int64_t)b * P;
  const int32_t* __restrict__ ib = path_b + (int64_t)b * P;
  float s1 = 0.f, s2 = 0.f;
  int c[5] = {0, 0, 0, 0, 0};
  for (int t = tid; t < n; t += 256) {
    const int i = ia[t], j = ib[t];
    if (i < 0 || i >= Fa || j < 0 || j >= Fb) continue;   // (not a cell of the tables: skipped, nothing is read for it)
    const float pa = ra[i], pb = rb[j];
    const bool va = pa > 0.f, vb = pb > 0.f;
    ++c[0];
    if (va && vb) {
      // formed in double and rounded once: two fp32 logarithms near 7 (1 ulp each on this hardware) would leave up to 1e-6 in a
      // difference below 3, which is the whole tolerance of a row with one voiced cell; at most 8 cells a thread
      const float x = (float)(log2((double)pb) - log2((double)pa));
      s1 += x;
      s2 += x * x;
      ++c[1];
      const float ga = gross * pa, gb = gross * pb;
      if (pa > gb || pb > ga) ++c[4];
    } else if (va) {
      ++c[2];
    } else if (vb) {
      ++c[3];
    }
  }
  red[0][tid] = s1;
  red[1][tid] = s2;
#pragma unroll
  for (int q = 0; q < 5; ++q) cnt[q][tid] = c[q];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
      red[0][tid] += red[0][tid + w];
      red[1][tid] += red[1][tid + w];
#pragma unroll
      for (int q = 0; q < 5; ++q) cnt[q][tid] += cnt[q][tid + w];
    }
    __syncthreads();
  }
  if (tid < 5) counts[5 * b + tid] = cnt[tid][0];
  if (tid == 0) {
    const int both = cnt[1][0];
    means[2 * b] = both > 0 ? red[0][0] / (float)both : 0.f;
    means[2 * b + 1] = both > 0 ? sqrtf(red[1][0] / (float)both) : 0.f;
  }
}

}  // namespace

extern "C" int taco_denorm_unframe(const float* out, const float* mean, const float* stdv, float* spec, float* mag_t, int B,
                                   int Td, int r, int C, void* stream) {
  TACO_REQUIRE(out && mean && stdv && (spec || mag_t) && B > 0 && Td > 0 && r >= 1 && r <= 5 && C > 0,
               "denorm_unframe: bad arguments");
  hipStream_t s = as_stream(stream);
  const int F = (Td / 4) * 4 * r;
  TACO_REQUIRE(F > 0, "denorm_unframe: Td=%d holds no whole chunk of 4 steps", Td);
  TACO_KLAUNCH(denorm_unframe_kernel, dim3((C + 31) / 32, (F + 31) / 32, B), dim3(32, 8), 0, s, out, mean, stdv, spec,
                     mag_t, Td, r, C, F);
  TACO_LAUNCH_CHECK("denorm_unframe");
  return TACO_OK;
}
namespace {
// refuses an output `name` of obytes bytes that overlaps the mbytes bytes of mag_t
int frames_no_overlap(const char* who, const char* name, const void* out, uint64_t obytes, const float* mag_t, uint64_t mbytes) {
  TACO_REQUIRE(!bytes_meet(out, obytes, mag_t, mbytes), "%s: %s overlaps mag_t", who, name);
  return TACO_OK;
}

// the refusals taco_frames_stretch and taco_frames_stretch_curve share, and the gather's grid
int frames_stretch_args(const char* who, const float* mag_t, const float* out, const int32_t* frames_out, int frames_per_unit, int B, int C,
                        int F, int Fo, int* nspan, int* ntile, int64_t* blocks) {
  TACO_REQUIRE(mag_t, "%s: mag_t is NULL", who);
  TACO_REQUIRE(out, "%s: out is NULL", who);
  TACO_REQUIRE(frames_out, "%s: frames_out is NULL", who);
  TACO_REQUIRE(B > 0, "%s: B=%d must be positive", who, B);
  TACO_REQUIRE(C > 0, "%s: C=%d must be positive", who, C);
  TACO_REQUIRE(F > 0 && F <= TACO_STRETCH_MAX_FRAMES, "%s: F=%d must be in 1..%d", who, F, TACO_STRETCH_MAX_FRAMES);
  TACO_REQUIRE(Fo > 0 && Fo <= TACO_STRETCH_MAX_FRAMES, "%s: Fo=%d must be in 1..%d", who, Fo, TACO_STRETCH_MAX_FRAMES);
  TACO_REQUIRE(frames_per_unit >= 1, "%s: frames_per_unit=%d must be >= 1", who, frames_per_unit);
  const uint64_t rows = (uint64_t)B * (uint64_t)C;   // (< 2^62; F, Fo <= 2^13: the byte counts below fit 64 bits)
  TACO_REQUIRE(rows <= (UINT64_MAX >> 16) / 4, "%s: B=%d x C=%d: the tensors exceed the address space", who, B, C);
  TACO_TRY(frames_no_overlap(who, "out", out, rows * Fo * 4, mag_t, rows * F * 4));
  *nspan = cdiv(Fo, kStretchSpan), *ntile = cdiv(C, kStretchBins);
  *blocks = (int64_t)B * *ntile * *nspan;
  TACO_REQUIRE(*blocks <= 0x7fffffff, "%s: B=%d x C=%d x Fo=%d needs more than 2^31 workgroups", who, B, C, Fo);
  return TACO_OK;
}

// the refusals of the entry points behind cepstrum_tile (taco_frames_pitch, _pitch_curve, _sharpen, _cepstats; `first`: the smallest
// lifter), and the grid
int frames_cepstrum_args(const char* who, const float* mag_t, int frames_per_unit, int first, int lifter, int B, int C, int F, int* ntile,
                         int64_t* blocks) {
  TACO_REQUIRE(mag_t, "%s: mag_t is NULL", who);
  TACO_REQUIRE(B > 0, "%s: B=%d must be positive", who, B);
  TACO_REQUIRE(C >= 9 && C <= kPitchMaxC && ((C - 1) & (C - 2)) == 0, "%s: C=%d: C - 1 must be a power of two in 8..%d", who, C,
               kPitchMaxC - 1);
  TACO_REQUIRE(F > 0 && F <= TACO_STRETCH_MAX_FRAMES, "%s: F=%d must be in 1..%d", who, F, TACO_STRETCH_MAX_FRAMES);
  const int qmax = (C - 1) / 2 < TACO_PITCH_MAX_LIFTER ? (C - 1) / 2 : TACO_PITCH_MAX_LIFTER;
  TACO_REQUIRE(lifter >= first && lifter <= qmax, "%s: lifter=%d must be in %d..%d at C=%d", who, lifter, first, qmax, C);
  TACO_REQUIRE(frames_per_unit >= 1, "%s: frames_per_unit=%d must be >= 1", who, frames_per_unit);
  *ntile = cdiv(F, kPitchFrames);
  *blocks = (int64_t)B * *ntile;
  TACO_REQUIRE(*blocks <= 0x7fffffff, "%s: B=%d x F=%d needs more than 2^31 workgroups", who, B, F);
  return TACO_OK;
}

// The two lifter paths of those kernels, chosen by the lifter alone (so the bits depend on it alone): launch(NB, kWaves) is called
// with <1, 16> for a lifter up to 32 and with <2, 8> above, as types that carry the numbers.
template <int V>
using int_c = std::integral_constant<int, V>;
template <class Launch>
void by_lifter(int lifter, Launch&& launch) {
  if (lifter <= 32) launch(int_c<1>{}, int_c<16>{});
  else launch(int_c<2>{}, int_c<8>{});
}

// taco_frames_pitch (CURVE = false: step_q (B)) and taco_frames_pitch_curve (true: step_q (B, F)): one set of refusals
template <bool CURVE>
int frames_pitch_call(const char* who, const float* mag_t, const int32_t* frames, int frames_per_unit, const int32_t* step_q, int lifter,
                      float* out, int B, int C, int F, void* stream) {
  int ntile;
  int64_t blocks;
  TACO_REQUIRE(!mag_t || out, "%s: out is NULL", who);   // (mag_t is refused first, below)
  TACO_TRY(frames_cepstrum_args(who, mag_t, frames_per_unit, 1, lifter, B, C, F, &ntile, &blocks));
  const uint64_t bytes = (uint64_t)B * (uint64_t)C * (uint64_t)F * 4;   // (< 2^31 * 2^11 * 2^13 * 4)
  TACO_TRY(frames_no_overlap(who, "out", out, bytes, mag_t, bytes));
  hipStream_t s = as_stream(stream);
  by_lifter(lifter, [&](auto nb, auto waves) {
    TACO_KLAUNCH((frames_pitch_kernel<nb.value, waves.value, CURVE>), dim3((unsigned)blocks), dim3(64 * waves.value), 0, s, mag_t, frames,
                 frames_per_unit, step_q, lifter, out, C, F, ntile);
  });
  TACO_LAUNCH_CHECK(who);
  return TACO_OK;
}
}  // namespace

extern "C" int taco_frames_sharpen(const float* mag_t, const int32_t* frames, int frames_per_unit, float beta, int lifter, float* out,
                                   int B, int C, int F, void* stream) {
  const char* who = "frames_sharpen";
  int ntile;
  int64_t blocks;
  TACO_REQUIRE(out, "%s: out is NULL", who);
  TACO_TRY(frames_cepstrum_args(who, mag_t, frames_per_unit, TACO_SHARPEN_FIRST, lifter, B, C, F, &ntile, &blocks));
  TACO_REQUIRE(beta >= TACO_SHARPEN_MIN_BETA && beta <= TACO_SHARPEN_MAX_BETA, "%s: beta=%g must be in [%g, %g]", who, (double)beta,
               (double)TACO_SHARPEN_MIN_BETA, (double)TACO_SHARPEN_MAX_BETA);   // (false for a NaN)
  const uint64_t bytes = (uint64_t)B * (uint64_t)C * (uint64_t)F * 4;   // (< 2^31 * 2^11 * 2^13 * 4)
  TACO_TRY(frames_no_overlap(who, "out", out, bytes, mag_t, bytes));
  hipStream_t s = as_stream(stream);
  by_lifter(lifter, [&](auto nb, auto waves) {
    TACO_KLAUNCH((frames_sharpen_kernel<nb.value, waves.value>), dim3((unsigned)blocks), dim3(64 * waves.value), 0, s, mag_t, frames,
                 frames_per_unit, beta, lifter, out, C, F, ntile);
  });
  TACO_LAUNCH_CHECK(who);
  return TACO_OK;
}
// workspace of taco_frames_cepstats: per tile of 32 frames (Q + 1) pairs of fp64
struct CepWs {
  double* partial;
  int64_t bytes;
};
static CepWs cep_ws(void* ws, int64_t blocks, int lifter) {
  WsCarver c(ws, 8);   // a workspace at any address: the base is rounded up
  CepWs w;
  w.partial = c.take<double>(blocks * (lifter + 1) * 2);
  c.take<char>(8);   // slack: the up to 7 bytes that rounding the base up costs
  w.bytes = c.bytes;
  return w;
}
extern "C" int64_t taco_frames_cepstats_workspace_bytes(int B, int C, int F, int lifter) {
  int ntile;
  int64_t blocks;
  const float dummy = 0.f;
  if (frames_cepstrum_args("frames_cepstats_workspace_bytes", &dummy, 1, TACO_SHARPEN_FIRST, lifter, B, C, F, &ntile, &blocks) != TACO_OK)
    return TACO_EINVAL;
  return cep_ws(nullptr, blocks, lifter).bytes;
}
extern "C" int taco_frames_cepstats(const float* mag_t, const int32_t* frames, int frames_per_unit, int lifter, double* sums,
                                    int32_t* count, void* workspace, int B, int C, int F, void* stream) {
  const char* who = "frames_cepstats";
  int ntile;
  int64_t blocks;
  TACO_REQUIRE(sums, "%s: sums is NULL", who);
  TACO_REQUIRE(count, "%s: count is NULL", who);
  TACO_TRY(frames_cepstrum_args(who, mag_t, frames_per_unit, TACO_SHARPEN_FIRST, lifter, B, C, F, &ntile, &blocks));
  TACO_REQUIRE(workspace, "%s: workspace is NULL", who);
  double* partial = cep_ws(workspace, blocks, lifter).partial;
  hipStream_t s = as_stream(stream);
  by_lifter(lifter, [&](auto nb, auto waves) {
    TACO_KLAUNCH((frames_cepstats_kernel<nb.value, waves.value>), dim3((unsigned)blocks), dim3(64 * waves.value), 0, s, mag_t, frames,
                 frames_per_unit, lifter, partial, C, F, ntile);
  });
  TACO_KLAUNCH(frames_cepstats_fold_kernel, dim3((unsigned)B), dim3(128), 0, s, partial, frames, frames_per_unit, lifter, sums, count, F,
               ntile);
  TACO_LAUNCH_CHECK(who);
  return TACO_OK;
}

extern "C" int taco_frames_stretch(const float* mag_t, const int32_t* frames, int frames_per_unit, const int32_t* step_q, float* out,
                                   int32_t* frames_out, int B, int C, int F, int Fo, void* stream) {
  int nspan, ntile;
  int64_t blocks;
  TACO_TRY(frames_stretch_args("frames_stretch", mag_t, out, frames_out, frames_per_unit, B, C, F, Fo, &nspan, &ntile, &blocks));
  hipStream_t s = as_stream(stream);
  TACO_KLAUNCH(frames_stretch_kernel<false>, dim3((unsigned)blocks), dim3(64, 4), 0, s, mag_t, frames, frames_per_unit, step_q, out,
               frames_out, C, F, Fo, nspan, ntile);
  TACO_LAUNCH_CHECK("frames_stretch");
  return TACO_OK;
}
// two launches on the caller's stream: the map (B workgroups), then the gather of taco_frames_stretch reading it
extern "C" int taco_frames_stretch_curve(const float* mag_t, const int32_t* frames, int frames_per_unit, const int32_t* dur_q, float* out,
                                         int32_t* frames_out, int32_t* src, int B, int C, int F, int Fo, void* stream) {
  int nspan, ntile;
  int64_t blocks;
  TACO_TRY(frames_stretch_args("frames_stretch_curve", mag_t, out, frames_out, frames_per_unit, B, C, F, Fo, &nspan, &ntile, &blocks));
  TACO_REQUIRE(src, "frames_stretch_curve: src is NULL");
  hipStream_t s = as_stream(stream);
  TACO_KLAUNCH(frames_stretch_map_kernel, dim3((unsigned)B), dim3(kMapThreads), 0, s, frames, frames_per_unit, dur_q, frames_out, src, F,
               Fo);
  TACO_KLAUNCH(frames_stretch_kernel<true>, dim3((unsigned)blocks), dim3(64, 4), 0, s, mag_t, nullptr, 1, src, out, frames_out, C, F, Fo,
               nspan, ntile);
  TACO_LAUNCH_CHECK("frames_stretch_curve");
  return TACO_OK;
}
extern "C" int taco_frames_pitch(const float* mag_t, const int32_t* frames, int frames_per_unit, const int32_t* step_q, int lifter,
                                 float* out, int B, int C, int F, void* stream) {
  return frames_pitch_call<false>("frames_pitch", mag_t, frames, frames_per_unit, step_q, lifter, out, B, C, F, stream);
}
extern "C" int taco_frames_pitch_curve(const float* mag_t, const int32_t* frames, int frames_per_unit, const int32_t* step_q, int lifter,
                                       float* out, int B, int C, int F, void* stream) {
  return frames_pitch_call<true>("frames_pitch_curve", mag_t, frames, frames_per_unit, step_q, lifter, out, B, C, F, stream);
}
// the refusals of taco_frames_pitch in its order
extern "C" int taco_frames_formant(const float* mag_t, const int32_t* frames, int frames_per_unit, const int32_t* step_q, int lifter,
                                   float* out, int B, int C, int F, void* stream) {
  const char* who = "frames_formant";
  int ntile;
  int64_t blocks;
  TACO_REQUIRE(!mag_t || out, "%s: out is NULL", who);   // (mag_t is refused first, below)
  TACO_TRY(frames_cepstrum_args(who, mag_t, frames_per_unit, 1, lifter, B, C, F, &ntile, &blocks));
  const uint64_t bytes = (uint64_t)B * (uint64_t)C * (uint64_t)F * 4;   // (< 2^31 * 2^11 * 2^13 * 4)
  TACO_TRY(frames_no_overlap(who, "out", out, bytes, mag_t, bytes));
  hipStream_t s = as_stream(stream);
  by_lifter(lifter, [&](auto nb, auto waves) {
    TACO_KLAUNCH((frames_formant_kernel<nb.value, waves.value>), dim3((unsigned)blocks), dim3(64 * waves.value), 0, s, mag_t, frames,
                 frames_per_unit, step_q, lifter, out, C, F, ntile);
  });
  TACO_LAUNCH_CHECK(who);
  return TACO_OK;
}
extern "C" int taco_frames_f0(const float* mag_t, const int32_t* frames, int frames_per_unit, const float* weight, const float* gain,
                              int lag_min, int lag_max, float ratio, float threshold, float* period, float* strength, float* acf,
                              int B, int C, int F, void* stream) {
  TACO_REQUIRE(mag_t, "frames_f0: mag_t is NULL");
  TACO_REQUIRE(period, "frames_f0: period is NULL");
  TACO_REQUIRE(strength, "frames_f0: strength is NULL");
  TACO_REQUIRE(B > 0, "frames_f0: B=%d must be positive", B);
  TACO_REQUIRE(C >= 9 && C <= kPitchMaxC && ((C - 1) & (C - 2)) == 0,
               "frames_f0: C=%d: C - 1 must be a power of two in 8..%d", C, kPitchMaxC - 1);
  TACO_REQUIRE(F > 0 && F <= TACO_STRETCH_MAX_FRAMES, "frames_f0: F=%d must be in 1..%d", F, TACO_STRETCH_MAX_FRAMES);
  TACO_REQUIRE(lag_min >= 2 && lag_min <= lag_max && lag_max <= C - 2,
               "frames_f0: lag_min=%d, lag_max=%d must satisfy 2 <= lag_min <= lag_max <= %d at C=%d", lag_min, lag_max, C - 2, C);
  const int L = lag_max - lag_min + 3;
  TACO_REQUIRE(L <= TACO_F0_MAX_LAGS, "frames_f0: lag_min=%d .. lag_max=%d are %d lags with their neighbours, at most %d", lag_min,
               lag_max, L, TACO_F0_MAX_LAGS);
  TACO_REQUIRE(ratio > 0.f && ratio <= 1.f, "frames_f0: ratio=%g must be in (0, 1]", (double)ratio);   // (NaN fails both)
  TACO_REQUIRE(threshold == threshold, "frames_f0: threshold is NaN");
  TACO_REQUIRE(frames_per_unit >= 1, "frames_f0: frames_per_unit=%d must be >= 1", frames_per_unit);
  const uint64_t mbytes = (uint64_t)B * (uint64_t)C * (uint64_t)F * 4, row = (uint64_t)B * (uint64_t)F * 4;
  TACO_TRY(frames_no_overlap("frames_f0", "period", period, row, mag_t, mbytes));
  TACO_TRY(frames_no_overlap("frames_f0", "strength", strength, row, mag_t, mbytes));
  if (acf) TACO_TRY(frames_no_overlap("frames_f0", "acf", acf, row * (uint64_t)L, mag_t, mbytes));
  const int ntile = cdiv(F, kF0Frames);
  const int64_t blocks = (int64_t)B * ntile;
  TACO_REQUIRE(blocks <= 0x7fffffff, "frames_f0: B=%d x F=%d needs more than 2^31 workgroups", B, F);
  hipStream_t s = as_stream(stream);
  if (L <= 32 * kF0Waves)
    TACO_KLAUNCH((frames_f0_kernel<1>), dim3((unsigned)blocks), dim3(64 * kF0Waves), 0, s, mag_t, frames, frames_per_unit, weight, gain,
                 lag_min, lag_max, ratio, threshold, period, strength, acf, C, F, ntile);
  else
    TACO_KLAUNCH((frames_f0_kernel<2>), dim3((unsigned)blocks), dim3(64 * kF0Waves), 0, s, mag_t, frames, frames_per_unit, weight, gain,
                 lag_min, lag_max, ratio, threshold, period, strength, acf, C, F, ntile);
  TACO_LAUNCH_CHECK("frames_f0");
  return TACO_OK;
}
extern "C" int taco_f0_stats(const float* period, const float* other, const int32_t* frames, int frames_per_unit, float* stats, int B,
                             int F, void* stream) {
  TACO_REQUIRE(period, "f0_stats: period is NULL");
  TACO_REQUIRE(stats, "f0_stats: stats is NULL");
  TACO_REQUIRE(B > 0, "f0_stats: B=%d must be positive", B);
  TACO_REQUIRE(F > 0 && F <= TACO_STRETCH_MAX_FRAMES, "f0_stats: F=%d must be in 1..%d", F, TACO_STRETCH_MAX_FRAMES);
  TACO_REQUIRE(frames_per_unit >= 1, "f0_stats: frames_per_unit=%d must be >= 1", frames_per_unit);
  TACO_KLAUNCH(f0_stats_kernel, dim3((unsigned)B), dim3(256), 0, as_stream(stream), period, other, frames, frames_per_unit, stats, F);
  TACO_LAUNCH_CHECK("f0_stats");
  return TACO_OK;
}
extern "C" int taco_path_f0_scores(const float* period_a, const float* period_b, const int32_t* path_a, const int32_t* path_b,
                                   const int32_t* steps, float gross, int32_t* counts, float* means, int B, int Fa, int Fb, void* stream) {
  TACO_REQUIRE(period_a && period_b, "path_f0_scores: period_a or period_b is NULL");
  TACO_REQUIRE(path_a && path_b, "path_f0_scores: path_a or path_b is NULL");
  TACO_REQUIRE(steps, "path_f0_scores: steps is NULL");
  TACO_REQUIRE(counts && means, "path_f0_scores: counts or means is NULL");
  TACO_REQUIRE(B > 0, "path_f0_scores: B=%d must be positive", B);
  TACO_REQUIRE(Fa > 0 && Fb > 0, "path_f0_scores: Fa=%d and Fb=%d must be positive", Fa, Fb);
  TACO_REQUIRE(Fa <= TACO_DTW_MAX_FRAMES && Fb <= TACO_DTW_MAX_FRAMES, "path_f0_scores: Fa=%d or Fb=%d is above the %d frames a row may have",
               Fa, Fb, TACO_DTW_MAX_FRAMES);
  TACO_REQUIRE(gross > 1.0f, "path_f0_scores: gross=%g must be above 1", (double)gross);   // (false for a NaN)
  TACO_KLAUNCH(path_f0_scores_kernel, dim3((unsigned)B), dim3(256), 0, as_stream(stream), period_a, period_b, path_a, path_b, steps, gross,
               counts, means, Fa, Fb);
  TACO_LAUNCH_CHECK("path_f0_scores");
  return TACO_OK;
}
