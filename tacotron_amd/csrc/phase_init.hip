// phase_init.hip -- initial phases for Griffin-Lim read off the magnitudes (include/taco_hip.h taco_phase_estimate): single-pass
// spectrogram inversion (Beauregard, Harish and Wyse 2015).  Every spectral peak of a frame is a sinusoid, its frequency refined by a
// parabola through three bins, its phase advanced by hop x frequency from the previous frame, the bins of its lobe locked to it.  No
// counterpart in the reference.  Integers and fp32 subtraction / multiplication / one IEEE division only: a NumPy restatement gives
// the same bits.  Two launches inside the one call.
//
// (a) Owners, parallel.  A workgroup of 4 waves owns 16 consecutive frames of a row.  The tile of |mag_t| goes through LDS as
// [bin][16 + 1] so that the global reads run along t (64 contiguous bytes per bin) and a wave's reads along the bins of one frame are
// free of bank conflicts (pitch 17).  A wave takes one frame at a time, lane l the bins l, 64 + l, ..., 17 words of 64 bins: the
// peak flags of a word are one ballot, so the frame's 1025 flags are 17 wave-uniform 64-bit masks.  The largest peak at or below a
// bin and the smallest above it then are a count-leading / count-trailing-zeros of the word under a lane mask, or -- where the word
// has no such bit -- the running last / first peak of the words in front of / behind it, two scalar loops over the 17 masks.  (No
// cross-lane scan is left: the ballots take the place of prefix-max / suffix-min scans by DPP and of their join through LDS.)  A
// bin then reads its owner's three magnitudes from the tile and forms the owner's advance itself.  Owner (int16, -1: none) and
// advance (uint32) go to the workspace frame-major, 1025 contiguous entries per frame.  Frames at and behind F_b are neither read
// nor written.
//
// (b) The chain, sequential.  One workgroup of 1024 threads per row walks t = 0 .. F_b - 1, thread i the bin i (thread 0 also bin
// 1024), the accumulators double-buffered in LDS: per frame one gather acc[own] + adv per bin and one barrier that waits for LDS
// only, so the records of the next kPeAhead frames stay in flight across it.  Sixteen waves, four per SIMD, because they cover each
// other's gather latency: with 256 threads and four bins each the chain took 1.02 us per frame, with these 0.61.  The
// phases collect in an LDS tile of 16 frames and go out transposed into (B, 1025, F) in runs of 64 bytes along t.  The same launch
// writes the zeros behind F_b.  No atomics, no flags, nothing polled: a row's chain lives inside its workgroup.
#include "frames.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int kPeBins = 1025;
constexpr int kPeWords = 17;                  // 64-bin words of a frame's peak flags
constexpr int kPeTile = 16;                   // frames per LDS tile, in both launches
constexpr int kPePitch = kPeTile + 1;
constexpr int kPeThreads = 256;
constexpr int kPeChainThreads = 1024;         // the chain: sixteen waves, four per SIMD, to cover each other's LDS and load latency
constexpr int kPeAhead = 4;                   // frames in flight per thread of the chain
constexpr int kPePer = 2;                     // bins per thread of the chain: tid, and bin 1024 for thread 0 only
constexpr size_t kPeTileLds = (size_t)kPeBins * kPePitch * 4;
constexpr size_t kPeChainLds = kPeTileLds + 2 * (size_t)kPeBins * 4;
constexpr size_t kPeLdsBudget = 96 * 1024;
constexpr float kPeScale = (float)(6.283185307179586 / 16777216.0);   // 2 pi / 2^24
static_assert(kPeWords * 64 >= kPeBins && (kPePer - 1) * kPeChainThreads + 1 == kPeBins, "bins per lane / per thread");
static_assert(kPeChainLds <= kPeLdsBudget, "LDS of the chain");

// steps 2 and 3 for the peak at bin j (1 <= j <= 1023) of the tile column `col`
__device__ __forceinline__ uint32_t pe_advance(const float* __restrict__ col, int j) {
  const float a = col[(j - 1) * kPePitch], b = col[j * kPePitch], c = col[(j + 1) * kPePitch];
  const float den = (a - 2.0f * b) + c;
  float p = 0.f;
  if (den != 0.f) p = fmaxf(-0.5f, fminf(0.5f, __fdiv_rn(0.5f * (a - c), den)));   // (a NaN becomes 0.5: nothing below is undefined)
  const int q = (int)rintf(p * 65536.0f);
  return (300u * (uint32_t)(j * 65536 + q)) << 5;   // wrapping: hop (j + p) / N turns in Q32
}

// ---- (a) owners ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPeThreads) void phase_owner_kernel(const float* __restrict__ mag_t, const int32_t* __restrict__ frames,
                                                                 int frames_per_unit, uint32_t* __restrict__ ws_adv,
                                                                 int16_t* __restrict__ ws_own, int F, int ntile) {
  extern __shared__ __attribute__((aligned(16))) float pe_lds[];   // |mag_t| [1025][17]
  float* tile = pe_lds;
  const int tl = (int)(blockIdx.x % (uint32_t)ntile), b = (int)(blockIdx.x / (uint32_t)ntile);
  const int Fb = row_frames_uniform(frames, frames_per_unit, b, F);
  const int f0 = tl * kPeTile;
  if (f0 >= Fb) return;   // (uniform) nothing of this tile is ever read
  const int tid = threadIdx.x;
  const int nf = min(kPeTile, Fb - f0);
  const float* __restrict__ src = mag_t + (int64_t)b * kPeBins * F + f0;
#pragma unroll 8
  for (int idx = tid; idx < kPeBins * kPeTile; idx += kPeThreads) {
    const int k = idx >> 4, tt = idx & (kPeTile - 1);
    if (tt < nf) tile[k * kPePitch + tt] = fabsf(src[(int64_t)k * F + tt]);
  }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  const uint64_t le = (2ull << lane) - 1ull;   // the bits of a word at or below this lane (lane 63: all)
  for (int tt = wave; tt < nf; tt += kPeThreads / 64) {   // (uniform per wave)
    const float* __restrict__ col = tile + tt;
    uint64_t bm[kPeWords];
    uint32_t rising = 0;
#pragma unroll
    for (int i = 0; i < kPeWords; ++i) {
      const int j = 64 * i + lane;
      bool peak = false;
      if (j + 1 < kPeBins) {
        const float m0 = col[j * kPePitch], mp = col[(j + 1) * kPePitch];
        if (mp > m0) rising |= 1u << i;
        if (j >= 1) peak = m0 > col[(j - 1) * kPePitch] && m0 >= mp;
      }
      bm[i] = __ballot(peak);
    }
    int before[kPeWords], behind[kPeWords];   // the last peak in front of word i / the first one behind it, -1: none
    int run = -1;
#pragma unroll
    for (int i = 0; i < kPeWords; ++i) {
      before[i] = run;
      if (bm[i]) run = 64 * i + 63 - __builtin_clzll(bm[i]);
    }
    run = -1;
#pragma unroll
    for (int i = kPeWords - 1; i >= 0; --i) {
      behind[i] = run;
      if (bm[i]) run = 64 * i + __builtin_ctzll(bm[i]);
    }
    const int64_t at = ((int64_t)b * F + f0 + tt) * kPeBins;
#pragma unroll
    for (int i = 0; i < kPeWords; ++i) {
      const int j = 64 * i + lane;
      if (j < kPeBins) {
        const uint64_t lo = bm[i] & le, hi = bm[i] & ~le;
        const int left = lo ? 64 * i + 63 - __builtin_clzll(lo) : before[i];
        const int right = hi ? 64 * i + __builtin_ctzll(hi) : behind[i];
        const int own = ((rising >> i) & 1u) ? right : left;   // (a peak does not rise: it owns itself)
        ws_adv[at + j] = own >= 0 ? pe_advance(col, own) : 0u;
        ws_own[at + j] = (int16_t)own;
      }
    }
  }
}

// ---- (b) the chain ------------------------------------------------------------------------------------------------------------------
struct PeRec {
  int o[kPePer];
  uint32_t a[kPePer];
};
__device__ __forceinline__ PeRec pe_load(const uint32_t* __restrict__ adv, const int16_t* __restrict__ own, int f, int last, int tid) {
  const int64_t at = (int64_t)min(f, last) * kPeBins;   // frames behind the row are read as its last one (written, never used)
  PeRec r;
#pragma unroll
  for (int i = 0; i < kPePer - 1; ++i) {
    r.o[i] = own[at + tid + kPeChainThreads * i];
    r.a[i] = adv[at + tid + kPeChainThreads * i];
  }
  r.o[kPePer - 1] = -1, r.a[kPePer - 1] = 0u;
  if (tid == 0) r.o[kPePer - 1] = own[at + kPeBins - 1], r.a[kPePer - 1] = adv[at + kPeBins - 1];
  return r;
}

__global__ __launch_bounds__(kPeChainThreads) void phase_chain_kernel(const uint32_t* __restrict__ ws_adv, const int16_t* __restrict__ ws_own,
                                                                 const int32_t* __restrict__ frames, int frames_per_unit,
                                                                 float* __restrict__ phase0, int F) {
  extern __shared__ __attribute__((aligned(16))) float pe_lds[];   // phases [1025][17] | accumulators [2][1025]
  float* tile = pe_lds;
  uint32_t* acc = reinterpret_cast<uint32_t*>(pe_lds + kPeBins * kPePitch);
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Fb = row_frames_uniform(frames, frames_per_unit, b, F);
  float* __restrict__ out = phase0 + (int64_t)b * kPeBins * F;
  if (Fb > 0) {   // (uniform)
    const int last = Fb - 1;
    const uint32_t* __restrict__ adv = ws_adv + (int64_t)b * F * kPeBins;
    const int16_t* __restrict__ own = ws_own + (int64_t)b * F * kPeBins;
    for (int j = tid; j < kPeBins; j += kPeChainThreads) acc[j] = 0u;
    PeRec ahead[kPeAhead];
#pragma unroll
    for (int k = 0; k < kPeAhead; ++k) ahead[k] = pe_load(adv, own, k, last, tid);
    lds_barrier();
    auto step = [&](const PeRec& now, int f) {
      const uint32_t* cur = acc + (f & 1) * kPeBins;
      uint32_t* nxt = acc + ((f + 1) & 1) * kPeBins;
      const int ft = f & (kPeTile - 1);
#pragma unroll
      for (int i = 0; i < kPePer; ++i) {
        if (i == kPePer - 1 && tid != 0) break;
        const int j = tid + kPeChainThreads * i;
        const int o = min(now.o[i], kPeBins - 1);   // (an owner is a bin; the reads do not rest on the workspace's contents)
        const uint32_t v = o >= 0 ? cur[o] + now.a[i] : cur[j];
        nxt[j] = v;
        const uint32_t u = (v + ((uint32_t)j << 31)) >> 8;   // half a turn per bin: the window is centred in its frame
        tile[j * kPePitch + ft] = (float)u * kPeScale;
      }
      lds_barrier();
      if (ft == kPeTile - 1 || f == last) {   // (uniform) the tile's frames f - ft .. f go out
        const int t0 = f - ft, nf = ft + 1;
        for (int idx = tid; idx < kPeBins * kPeTile; idx += kPeChainThreads) {
          const int k = idx >> 4, tt = idx & (kPeTile - 1);
          if (tt < nf) out[(int64_t)k * F + t0 + tt] = tile[k * kPePitch + tt];
        }
        lds_barrier();   // (the next frame writes the tile again)
      }
    };
    for (int f = 0; f < Fb; f += kPeAhead) {
#pragma unroll
      for (int k = 0; k < kPeAhead; ++k) {
        if (f + k >= Fb) break;   // (uniform)
        const PeRec now = ahead[k];
        ahead[k] = pe_load(adv, own, f + k + kPeAhead, last, tid);
        step(now, f + k);
      }
    }
  }
  if (Fb < F) {
    for (int k = 0; k < kPeBins; ++k)
      for (int t = Fb + tid; t < F; t += kPeChainThreads) out[(int64_t)k * F + t] = 0.f;
  }
}

// workspace of taco_phase_estimate: the advances (uint32) and the owners (int16), frame-major, 1025 entries per frame
struct PeWs {
  uint32_t* adv;
  int16_t* own;
  int64_t bytes;
};
PeWs pe_ws(void* ws, int B, int F) {
  WsCarver c(ws);
  PeWs w;
  const int64_t n = (int64_t)B * F * kPeBins;
  w.adv = c.take<uint32_t>(n);
  w.own = c.take<int16_t>(n);
  c.take<char>(0, 4);   // the size is a whole number of 4-byte words (B F odd: 2 bytes behind the owners)
  w.bytes = c.bytes;
  return w;
}

}  // namespace

extern "C" int64_t taco_phase_estimate_workspace_bytes(int B, int F) {
  if (B <= 0 || F <= 0) return TACO_EINVAL;
  return pe_ws(nullptr, B, F).bytes;
}

extern "C" int taco_phase_estimate(const float* mag_t, const int32_t* frames, int frames_per_unit, float* phase0, void* workspace, int B,
                                   int F, void* stream) {
  TACO_REQUIRE(mag_t, "phase_estimate: mag_t is NULL");
  TACO_REQUIRE(phase0, "phase_estimate: phase0 is NULL");
  TACO_REQUIRE(workspace, "phase_estimate: workspace is NULL (owners and advances need taco_phase_estimate_workspace_bytes bytes)");
  TACO_REQUIRE(B > 0, "phase_estimate: B=%d must be positive", B);
  TACO_REQUIRE(F > 0, "phase_estimate: F=%d must be positive", F);
  TACO_REQUIRE(frames_per_unit >= 1, "phase_estimate: frames_per_unit=%d must be >= 1", frames_per_unit);
  const uint64_t bytes = (uint64_t)B * F * kPeBins * 4;
  TACO_REQUIRE(!bytes_meet(phase0, bytes, mag_t, bytes), "phase_estimate: phase0 overlaps mag_t");
  const int ntile = cdiv(F, kPeTile);
  const int64_t blocks = (int64_t)B * ntile;
  TACO_REQUIRE(blocks <= 0x7fffffff, "phase_estimate: B=%d x F=%d needs more than 2^31 workgroups", B, F);
  static DynSmemOnce owner_raised, chain_raised;
  if (!ensure_dyn_smem(owner_raised, reinterpret_cast<const void*>(phase_owner_kernel), kPeLdsBudget) ||
      !ensure_dyn_smem(chain_raised, reinterpret_cast<const void*>(phase_chain_kernel), kPeLdsBudget)) {
    taco_set_error("phase_estimate: cannot raise the dynamic LDS limit to %zu bytes", kPeLdsBudget);
    return TACO_ELAUNCH;
  }
  hipStream_t s = as_stream(stream);
  const PeWs w = pe_ws(workspace, B, F);
  uint32_t* ws_adv = w.adv;
  int16_t* ws_own = w.own;
  TACO_KLAUNCH(phase_owner_kernel, dim3((unsigned)blocks), dim3(kPeThreads), kPeTileLds, s, mag_t, frames, frames_per_unit, ws_adv, ws_own,
               F, ntile);
  TACO_KLAUNCH(phase_chain_kernel, dim3((unsigned)B), dim3(kPeChainThreads), kPeChainLds, s, ws_adv, ws_own, frames, frames_per_unit, phase0, F);
  TACO_LAUNCH_CHECK("phase_estimate");
  return TACO_OK;
}
