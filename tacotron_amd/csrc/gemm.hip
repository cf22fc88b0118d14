// gemm.hip -- fp32 MFMA (v_mfma_f32_32x32x2_f32) GEMM family for the feed-forward part of the Tacotron hot path.
//
//   conv_gemm (NN): C = post(act(sum_tap shift_tap(A) . W[tap] + bias))  -- tf.layers.dense (tacotron.py:40-43,148),
//                   tf.layers.conv1d 'same' (ops.py:54-60,80-86), hoisted GRU input projections (ops.py:117-128),
//                   and (with pre-transposed weights) every activation gradient dA = dZ . W^T.
//   gemm_tn       : dW[tap] += shift_tap(A)^T . dY              -- every weight gradient (tacotron.py:172).
//
// Tiling: 256 threads = 4 waves (2x2), each wave WMxWN 32x32 MFMA tiles; block tile (64*WM) x (64*WN), BK = 16.
// A/B tiles are staged k-major in LDS so that the f32 MFMA operand fetch (lane l -> [k = l>>5][i = l&31]) is a
// conflict-free 32-lane contiguous ds_read_b32.  Global loads are float4 along the contiguous dimension with a
// scalar fallback for unaligned leading dimensions (e.g. 1025-wide linear frames).
#include <algorithm>

#include "bf16x3.h"
#include "common.h"
#include "kernels.h"

namespace {

constexpr int BK = 16;

// component-wise select (a struct-level `ok ? t : zero` is lowered through scratch memory by hipcc)
__device__ __forceinline__ float4 sel4(bool ok, const float4 t) {
  return make_float4(ok ? t.x : 0.f, ok ? t.y : 0.f, ok ? t.z : 0.f, ok ? t.w : 0.f);
}

struct RowInfo {
  int m;      // global output row
  int t;      // position inside its sequence
  bool ok;    // m < M
};

// VA / VB: the A / W operand satisfies the vector-load contract (16-byte aligned base and leading dimension, K resp.
// N a multiple of 4, or padded storage declared through Kld / Nld) -> branch-free float4 loads whose waits the
// compiler can sink below the MFMA block.  The scalar fallback keeps exact bounds checks for odd test shapes.
template <int WM, int WN, bool VA, bool VB>
__global__ __launch_bounds__(256) void conv_gemm_kernel(ConvGemmBatch batch) {
  constexpr int BM = 64 * WM, BN = 64 * WN;
  constexpr int LDS_A = BM + 4, LDS_B = BN + 4;
  constexpr int A_PER = BM / 64;   // float4 loads of A per thread per tile  (BM rows x 4 float4)
  constexpr int B_PER = BN / 64;   // float4 loads of W per thread per tile  (16 rows x BN/4 float4)
  const ConvGemmProblem& P = batch.p[blockIdx.z];
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  if (m0 >= P.M || n0 >= P.N) return;

  __shared__ __attribute__((aligned(16))) float As[2][BK][LDS_A];
  __shared__ __attribute__((aligned(16))) float Bs[2][BK][LDS_B];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;

  // --- loader mapping ---
  const int a_kq = tid & 3;          // which float4 along k (4 per row)
  const int a_row = tid >> 2;        // 0..63 (+64*i)
  RowInfo ar[A_PER];
#pragma unroll
  for (int i = 0; i < A_PER; ++i) {
    int m = m0 + a_row + 64 * i;
    ar[i].m = m;
    ar[i].ok = m < P.M;
    ar[i].t = ar[i].ok ? (m % P.T) : 0;
  }
  constexpr int B_COLS4 = BN / 4;            // float4 per W row
  const int b_c4 = tid % B_COLS4;
  const int b_k = tid / B_COLS4;             // 0 .. 256/B_COLS4-1
  constexpr int B_KSTEP = 256 / B_COLS4;     // rows covered per pass (8 for BN=128, 16 for BN=64)

  const int ktiles = (P.K + BK - 1) / BK;
  const int nit = P.taps * ktiles;

  // One k-tile in flight: raw float4s plus (VEC paths) their validity, applied when the tile is written to LDS.  TWO stages
  // alternate, so a tile is fetched two iterations before it is stored: with 64x64 tiles an iteration is 8 MFMAs per wave
  // (512 matrix-pipe cycles), shorter than an L2 round trip, and a one-deep prefetch stalled every iteration.
  struct Stage {
    float4 ra[A_PER], rb[B_PER];
    bool oka[A_PER], okb[B_PER];
  };
  Stage st0, st1;

  auto load_tile = [&](Stage& S, int it) {
    const int tap = it / ktiles;
    const int k0 = (it - tap * ktiles) * BK;
    const int sh = tap - P.pad_l;
#pragma unroll
    for (int i = 0; i < A_PER; ++i) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      const int st = ar[i].t + sh;
      const int k = k0 + a_kq * 4;
      if constexpr (VA) {
        const bool ok = ar[i].ok && (unsigned)st < (unsigned)P.T && k < P.K;
        const int64_t off = (int64_t)ok * ((int64_t)(ar[i].m + sh) * P.lda + k);
        v = *reinterpret_cast<const float4*>(P.A + off);
        S.oka[i] = ok;
      } else if (ar[i].ok && st >= 0 && st < P.T) {
        const float* p = P.A + (int64_t)(ar[i].m + sh) * P.lda + k;
        if (k < P.K) v.x = p[0];
        if (k + 1 < P.K) v.y = p[1];
        if (k + 2 < P.K) v.z = p[2];
        if (k + 3 < P.K) v.w = p[3];
      }
      S.ra[i] = v;
    }
    const float* Wt = P.W + (int64_t)tap * P.K * P.ldw;
#pragma unroll
    for (int i = 0; i < B_PER; ++i) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      const int k = k0 + b_k + i * B_KSTEP;
      const int n = n0 + b_c4 * 4;
      if constexpr (VB) {
        const bool ok = k < P.K && n < P.Nld;
        const int64_t off = (int64_t)ok * ((int64_t)k * P.ldw + n);
        v = *reinterpret_cast<const float4*>(Wt + off);
        S.okb[i] = ok;
      } else if (k < P.K) {
        const float* p = Wt + (int64_t)k * P.ldw + n;
        if (n < P.N) v.x = p[0];
        if (n + 1 < P.N) v.y = p[1];
        if (n + 2 < P.N) v.z = p[2];
        if (n + 3 < P.N) v.w = p[3];
      }
      S.rb[i] = v;
    }
  };
  auto store_tile = [&](const Stage& S, int buf) {
#pragma unroll
    for (int i = 0; i < A_PER; ++i) {
      const int r = a_row + 64 * i;
      const float4 v = VA ? sel4(S.oka[i], S.ra[i]) : S.ra[i];
      As[buf][a_kq * 4 + 0][r] = v.x;
      As[buf][a_kq * 4 + 1][r] = v.y;
      As[buf][a_kq * 4 + 2][r] = v.z;
      As[buf][a_kq * 4 + 3][r] = v.w;
    }
#pragma unroll
    for (int i = 0; i < B_PER; ++i) {
      const int k = b_k + i * B_KSTEP;
      if (k < BK) *reinterpret_cast<float4*>(&Bs[buf][k][b_c4 * 4]) = VB ? sel4(S.okb[i], S.rb[i]) : S.rb[i];
    }
  };

  f32x16 acc[WM][WN];
#pragma unroll
  for (int i = 0; i < WM; ++i)
#pragma unroll
    for (int j = 0; j < WN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  load_tile(st0, 0);
  store_tile(st0, 0);
  if (1 < nit) load_tile(st1, 1);   // tile 1 -> stage 1, tile 2 -> stage 0
  if (2 < nit) load_tile(st0, 2);
  __syncthreads();

  const int lk = lane >> 5, li = lane & 31;
  auto compute = [&](int buf) {
    // LDS operands are fetched one k-pair ahead of the MFMAs that consume them
      float a[2][WM], b[2][WN];
#pragma unroll
      for (int i = 0; i < WM; ++i) a[0][i] = As[buf][lk][wm * (32 * WM) + i * 32 + li];
#pragma unroll
      for (int j = 0; j < WN; ++j) b[0][j] = Bs[buf][lk][wn * (32 * WN) + j * 32 + li];
#pragma unroll
      for (int kk = 0; kk < BK; kk += 2) {
        const int cur = (kk >> 1) & 1, nxt = cur ^ 1;
        if (kk + 2 < BK) {
#pragma unroll
          for (int i = 0; i < WM; ++i) a[nxt][i] = As[buf][kk + 2 + lk][wm * (32 * WM) + i * 32 + li];
#pragma unroll
          for (int j = 0; j < WN; ++j) b[nxt][j] = Bs[buf][kk + 2 + lk][wn * (32 * WN) + j * 32 + li];
        }
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
          for (int j = 0; j < WN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cur][i], b[cur][j], acc[i][j], 0, 0, 0);
      }
  };
  // iteration it computes on LDS buffer it & 1, stores tile it+1 (stage (it+1) & 1, fetched two iterations ago) into the other
  // buffer and refills that stage with tile it+3
  for (int it = 0; it < nit; it += 2) {
    compute(0);
    if (it + 1 < nit) store_tile(st1, 1);
    if (it + 3 < nit) load_tile(st1, it + 3);
    __syncthreads();
    if (it + 1 < nit) {
      compute(1);
      if (it + 2 < nit) store_tile(st0, 0);
      if (it + 4 < nit) load_tile(st0, it + 4);
      __syncthreads();
    }
  }

  // --- epilogue: C/D layout col = lane&31, row = (e&3) + 8*(e>>2) + 4*(lane>>5) ---
#pragma unroll
  for (int i = 0; i < WM; ++i) {
#pragma unroll
    for (int j = 0; j < WN; ++j) {
      const int n = n0 + wn * (32 * WN) + j * 32 + li;
      if (n >= P.N) continue;
      const float bias0 = (P.bias && P.bias_stride == 0) ? P.bias[n] : 0.f;
      const float sc = P.scale ? P.scale[n] * P.scale_mul : 1.f;
      const float sf = P.shift ? P.shift[n] : 0.f;
      // Three passes over the 16 elements: every epilogue operand is LOADED (raw: no arithmetic on a loaded value inside the
      // load pass), then everything is computed, then everything is stored.  Written as one loop -- load, compute, store per
      // element -- each use of a loaded register behind the previous element's conditional store is an `s_waitcnt vmcnt(0)`,
      // i.e. a wait for that store's acknowledgement: 16 serial round trips per accumulator tile (measured on prenet.hip:
      // 17 us of a 45 us workgroup).
      const int mrow = m0 + wm * (32 * WM) + i * 32 + 4 * lk;
      float bias_e[16], res_e[16];
      unsigned keep_e[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) bias_e[e] = bias0, res_e[e] = 0.f, keep_e[e] = 1u;
      if (P.bias_stride) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int m = min(mrow + (e & 3) + 8 * (e >> 2), P.M - 1);
          bias_e[e] = P.bias[(int64_t)(m / P.T) * P.bias_stride + n];
        }
      }
      if (P.keep) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int m = min(mrow + (e & 3) + 8 * (e >> 2), P.M - 1);
          keep_e[e] = P.keep[(int64_t)m * P.N + n];
        }
      }
      if (P.residual) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int m = min(mrow + (e & 3) + 8 * (e >> 2), P.M - 1);
          res_e[e] = P.residual[(int64_t)m * P.ldr + n];
        }
      }
      float pre_e[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        float v = apply_act(acc[i][j][e] + bias_e[e], P.act);
        if (P.keep) v = keep_e[e] ? v * 2.0f : 0.0f;
        pre_e[e] = v;
        if (P.scale || P.shift) v = v * sc + sf;
        acc[i][j][e] = v + res_e[e];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int m = mrow + (e & 3) + 8 * (e >> 2);
        if (m >= P.M) continue;
        if (P.Cpre) P.Cpre[(int64_t)m * P.ldc + n] = pre_e[e];
        if (P.atomic_out) atomicAdd(&P.C[(int64_t)m * P.ldc + n], acc[i][j][e]);
        else P.C[(int64_t)m * P.ldc + n] = acc[i][j][e];
      }
    }
  }
}

// second pass of launch_conv_gemm_tapsplit: C = epilogue(slab_0 + slab_1 + ... in tap order); 4 columns per thread
__global__ void conv_gemm_tapsum_kernel(ConvGemmProblem P, const float* __restrict__ slabs, int taps) {
  const int64_t total4 = (int64_t)P.M * P.N / 4;
  const int64_t slab = (int64_t)P.M * P.N;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (int64_t)gridDim.x * blockDim.x) {
    const int m = (int)(i * 4 / P.N), n0 = (int)(i * 4 - (int64_t)m * P.N);
    float4 s = reinterpret_cast<const float4*>(slabs)[i];
    for (int t = 1; t < taps; ++t) {
      const float4 v = reinterpret_cast<const float4*>(slabs + t * slab)[i];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    float r[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + j;
      const float bias = P.bias ? (P.bias_stride ? P.bias[(int64_t)(m / P.T) * P.bias_stride + n] : P.bias[n]) : 0.f;
      float v = apply_act(r[j] + bias, P.act);
      if (P.keep) v = P.keep[(int64_t)m * P.N + n] ? v * 2.0f : 0.0f;
      if (P.Cpre) P.Cpre[(int64_t)m * P.ldc + n] = v;
      if (P.scale || P.shift) v = v * (P.scale ? P.scale[n] * P.scale_mul : 1.f) + (P.shift ? P.shift[n] : 0.f);
      if (P.residual) v += P.residual[(int64_t)m * P.ldr + n];
      if (P.atomic_out) P.C[(int64_t)m * P.ldc + n] += v;   // "C += result": one thread owns the element, no atomic needed
      else P.C[(int64_t)m * P.ldc + n] = v;
    }
  }
}

// dW[z][tap][k][n] += sum_m A[z][row(m,tap)][k] * dY[z][m][n]; reduction over m split across blockIdx.z slices.
// BX: the products on the bf16 matrix pipe (bf16x3.h): the lane's 8 row slots of a 16-row tile are m = 2 q + lk, the same sixteen
// ds_read_b32 per operand sub-tile as the fp32 form; every operand sub-tile is split into three bf16 planes in registers and a
// 32 x 32 output sub-tile takes six v_mfma_f32_32x32x16_bf16 per tile instead of eight v_mfma_f32_32x32x2_f32.
template <int WM, int WN, bool VA, bool VB, bool BX = false>
__device__ __forceinline__ void gemm_tn_body(const GemmTnArgs& P, const int bx, const int by, const int bz_) {
  constexpr int BM = 64 * WM, BN = 64 * WN;   // BM tiles the k (output row) dimension
  constexpr int LDS_A = BM + 4, LDS_B = BN + 4;
  constexpr int A_PER = BM / 64, B_PER = BN / 64;
  const int k0 = bx * BM, n0 = by * BN;
  int z = bz_;
  const int split = z % P.splits;
  z /= P.splits;
  const int tap = z % P.taps;
  const int bz = z / P.taps;
  const float* A = P.A + (int64_t)bz * P.strideA;
  const float* Y = P.Y + (int64_t)bz * P.strideY;
  float* W = P.W + (int64_t)bz * P.strideW + (int64_t)tap * P.K * P.ldw;

  __shared__ __attribute__((aligned(16))) float As[2][BK][LDS_A];
  __shared__ __attribute__((aligned(16))) float Bs[2][BK][LDS_B];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int sh = tap - P.pad_l;

  constexpr int A_COLS4 = BM / 4, B_COLS4 = BN / 4;
  constexpr int A_RSTEP = 256 / A_COLS4, B_RSTEP = 256 / B_COLS4;
  const int a_c4 = tid % A_COLS4, a_r = tid / A_COLS4;
  const int b_c4 = tid % B_COLS4, b_r = tid / B_COLS4;

  const int m_begin = split * P.chunk;
  const int m_end = min(P.M, m_begin + P.chunk);
  const int nit = (m_end - m_begin + BK - 1) / BK;
  if (nit <= 0) return;

  float4 ra[A_PER], rb[B_PER];
  const bool do_bias = P.dbias != nullptr && bx == 0 && tap == 0;
  float4 bsum[B_PER];
#pragma unroll
  for (int i = 0; i < B_PER; ++i) bsum[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  // Vector paths (round 4): both operands through buffer descriptors.  A lane's byte offset is fixed for the launch, the row
  // advance of a tile is the instruction's SGPR offset, a masked lane (rows outside the chunk / outside their sequence for a
  // shifted tap, the K / N tails) carries an out-of-range offset and receives zeros, and the row-in-sequence index is carried
  // from tile to tile instead of a modulo per load (the modulo alone was 5-9 % of the big launches, profiles/r04_tn_lab.txt).
  // The launcher only sets the vector flags when both operands are addressable with 31 bits.
  constexpr int kOOB = (int)0x80000000;
  __amdgpu_buffer_rsrc_t rsA, rsY;
  int a_vo[A_PER], a_t[A_PER], b_vo[B_PER];
  int sh_t = sh;   // row shift of this thread's A columns (merged taps: the tap its columns belong to)
  if constexpr (VA) {
    int kcol = k0 + a_c4 * 4;
    if (P.ktap > 0) {
      const int tc = kcol / P.ktap;
      kcol -= tc * P.ktap;
      sh_t = tc - P.pad_l;
    }
    // (the descriptor starts 16 rows in front of A so that a negative shift keeps the byte offset positive; rows outside their
    //  sequence are masked by `ok` below whatever the offset)
    rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(A - (int64_t)16 * P.lda), 0, 0x7fffffff, 0x00020000);
#pragma unroll
    for (int i = 0; i < A_PER; ++i) {
      const int r = a_r + i * A_RSTEP, k = k0 + a_c4 * 4;
      a_vo[i] = (r < BK && k < P.K) ? ((m_begin + r + sh_t + 16) * P.lda + kcol) * 4 : kOOB;
      a_t[i] = (m_begin + r) % P.T;
    }
  }
  if constexpr (VB) {
    rsY = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Y), 0, 0x7fffffff, 0x00020000);
#pragma unroll
    for (int i = 0; i < B_PER; ++i) {
      const int r = b_r + i * B_RSTEP, n = n0 + b_c4 * 4;
      b_vo[i] = (r < BK && n < P.Nld) ? ((m_begin + r) * P.ldy + n) * 4 : kOOB;
    }
  }
  auto as_f4 = [](auto v) { return __builtin_bit_cast(float4, v); };
  auto load_tile = [&](int it) {   // called with it = 0, 1, 2, ... in order (a_t is carried)
    const int mm0 = m_begin + it * BK;
#pragma unroll
    for (int i = 0; i < A_PER; ++i) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      const int r = a_r + i * A_RSTEP;
      const int m = mm0 + r;
      const int k = k0 + a_c4 * 4;
      if constexpr (VA) {
        const bool ok = m < m_end && (unsigned)(a_t[i] + sh_t) < (unsigned)P.T;
        v = as_f4(__builtin_amdgcn_raw_buffer_load_b128(rsA, ok ? a_vo[i] : kOOB, it * (BK * 4) * P.lda, 0));
        a_t[i] += BK;
        if (P.T >= BK) a_t[i] = a_t[i] >= P.T ? a_t[i] - P.T : a_t[i];
        else a_t[i] %= P.T;
      } else if (r < BK && m < m_end) {
        const int st = (m % P.T) + sh;
        if (st >= 0 && st < P.T) {
          const float* p = A + (int64_t)(m + sh) * P.lda + k;
          if (k < P.K) v.x = p[0];
          if (k + 1 < P.K) v.y = p[1];
          if (k + 2 < P.K) v.z = p[2];
          if (k + 3 < P.K) v.w = p[3];
        }
      }
      ra[i] = v;
    }
#pragma unroll
    for (int i = 0; i < B_PER; ++i) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      const int r = b_r + i * B_RSTEP;
      const int m = mm0 + r;
      const int n = n0 + b_c4 * 4;
      if constexpr (VB) {
        v = as_f4(__builtin_amdgcn_raw_buffer_load_b128(rsY, m < m_end ? b_vo[i] : kOOB, it * (BK * 4) * P.ldy, 0));
      } else if (r < BK && m < m_end) {
        const float* p = Y + (int64_t)m * P.ldy + n;
        if (n < P.N) v.x = p[0];
        if (n + 1 < P.N) v.y = p[1];
        if (n + 2 < P.N) v.z = p[2];
        if (n + 3 < P.N) v.w = p[3];
      }
      rb[i] = v;
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int i = 0; i < A_PER; ++i) {
      const int r = a_r + i * A_RSTEP;
      if (r < BK) *reinterpret_cast<float4*>(&As[buf][r][a_c4 * 4]) = ra[i];
    }
#pragma unroll
    for (int i = 0; i < B_PER; ++i) {
      const int r = b_r + i * B_RSTEP;
      const float4 v = rb[i];
      if (r < BK) *reinterpret_cast<float4*>(&Bs[buf][r][b_c4 * 4]) = v;
      if (do_bias) { bsum[i].x += v.x; bsum[i].y += v.y; bsum[i].z += v.z; bsum[i].w += v.w; }
    }
  };

  f32x16 acc[WM][WN];
#pragma unroll
  for (int i = 0; i < WM; ++i)
#pragma unroll
    for (int j = 0; j < WN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  f32x16 acc_lo[BX ? WM : 1][BX ? WN : 1];   // bf16x3: the low-order plane products' own accumulators (bf16x3.h mfma6_2)
#pragma unroll
  for (int i = 0; i < (BX ? WM : 1); ++i)
#pragma unroll
    for (int j = 0; j < (BX ? WN : 1); ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc_lo[i][j][e] = 0.f;

  load_tile(0);
  store_tile(0);
  __syncthreads();
  const int lk = lane >> 5, li = lane & 31;
  for (int it = 0; it < nit; ++it) {
    const int buf = it & 1;
    if (it + 1 < nit) load_tile(it + 1);
    if constexpr (BX) {
      static_assert(BK == 16, "one v_mfma_f32_32x32x16_bf16 group per 16-row tile");
      Pl3 pa[WM], pb[WN];
#pragma unroll
      for (int i = 0; i < WM; ++i) {
        float f[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) f[q] = As[buf][2 * q + lk][wm * (32 * WM) + i * 32 + li];
        pa[i] = split8(f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7]);
      }
#pragma unroll
      for (int j = 0; j < WN; ++j) {
        float f[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) f[q] = Bs[buf][2 * q + lk][wn * (32 * WN) + j * 32 + li];
        pb[j] = split8(f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7]);
      }
#pragma unroll
      for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j) {
          mfma6_2(acc[i][j], acc_lo[i][j], pa[i], pb[j]);
        }
      if (it + 1 < nit) store_tile(buf ^ 1);
      __syncthreads();
      continue;
    }
    // LDS operands are fetched one k-pair ahead of the MFMAs that consume them
    float a[2][WM], b[2][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i) a[0][i] = As[buf][lk][wm * (32 * WM) + i * 32 + li];
#pragma unroll
    for (int j = 0; j < WN; ++j) b[0][j] = Bs[buf][lk][wn * (32 * WN) + j * 32 + li];
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2) {
      const int cur = (kk >> 1) & 1, nxt = cur ^ 1;
      if (kk + 2 < BK) {
#pragma unroll
        for (int i = 0; i < WM; ++i) a[nxt][i] = As[buf][kk + 2 + lk][wm * (32 * WM) + i * 32 + li];
#pragma unroll
        for (int j = 0; j < WN; ++j) b[nxt][j] = Bs[buf][kk + 2 + lk][wn * (32 * WN) + j * 32 + li];
      }
#pragma unroll
      for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cur][i], b[cur][j], acc[i][j], 0, 0, 0);
    }
    if (it + 1 < nit) store_tile(buf ^ 1);
    __syncthreads();
  }

  if constexpr (BX) {
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
      for (int j = 0; j < WN; ++j) acc[i][j] += acc_lo[i][j];
  }
#pragma unroll
  for (int i = 0; i < WM; ++i) {
#pragma unroll
    for (int j = 0; j < WN; ++j) {
      const int n = n0 + wn * (32 * WN) + j * 32 + li;
      if (n >= P.N) continue;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int k = k0 + wm * (32 * WM) + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lk;
        if (k >= P.K) continue;
        atomicAdd(&W[(int64_t)k * P.ldw + n], acc[i][j][e]);
      }
    }
  }
  if (do_bias) {
    // column sums of this block's Y rows: per-thread partials -> LDS rows (As is free after the last barrier) -> summed in row
    // order (no LDS atomics: the order of the adds is fixed)
    float* cs = &As[0][0][0];
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < B_PER; ++i) { t.x += bsum[i].x; t.y += bsum[i].y; t.z += bsum[i].z; t.w += bsum[i].w; }
    __syncthreads();
    *reinterpret_cast<float4*>(&cs[b_r * LDS_B + b_c4 * 4]) = t;   // B_RSTEP (8 or 16) rows of BN partial sums
    __syncthreads();
    float* db = P.dbias + (int64_t)bz * P.N;
    for (int i = tid; i < BN; i += 256) {
      float c = 0.f;
      for (int r = 0; r < B_RSTEP; ++r) c += cs[r * LDS_B + i];
      if (n0 + i < P.N) atomicAdd(&db[n0 + i], c);   // one contribution per launch in deterministic mode (splits == 1)
    }
  }
}

// XCD-aware block order of the weight-gradient launches (round 5).  The dispatcher deals consecutive workgroups round-robin to the 8
// XCDs, so the gx * gy output tiles of ONE row-range slice z -- which all read the same rows of A and dY -- used to be spread over
// all eight L2s: every L2 fetched (nearly) every slice, up to 8 x the operand bytes over the fabric (profiles/r05_pmc_step.txt:
// 2.75 GB fetched per step by these kernels for ~0.4 GB of operands).  With this order slice z is worked on by XCD z % 8 alone: the
// s-th workgroup that lands on XCD x takes tile s % per of slice x + 8 (s / per).  Slices beyond the last multiple of 8 keep the
// plain order.  L: linear workgroup index within the problem (its first workgroup is at a multiple of 8 of the grid).
__device__ __forceinline__ void tn_xcd_order(int L, int per, int gz, bool on, int& t, int& z) {
  const int zfull = gz & ~7;
  if (on && L < per * zfull) {
    const int x = L & 7, s = L >> 3;
    const int g = s / per;
    z = x + 8 * g;
    t = s - g * per;
  } else {
    z = L / per;
    t = L - z * per;
  }
}

template <int WM, int WN, bool VA, bool VB, bool BX = false>
__global__ __launch_bounds__(256) void gemm_tn_kernel(GemmTnArgs P) {
  const int gx = gridDim.x, per = gx * gridDim.y;
  int t, z;
  tn_xcd_order(blockIdx.x + gx * (blockIdx.y + gridDim.y * blockIdx.z), per, gridDim.z, P.xcd != 0, t, z);
  const int by = t / gx;
  gemm_tn_body<WM, WN, VA, VB, BX>(P, t - by * gx, by, z);
}

// Grouped launch: independent weight-gradient GEMMs (all 64x64 tiles, vector contract) share ONE grid; block -> problem
// by a prefix table of block counts, so ~20 launch-latency-sized GEMMs run concurrently instead of back to back.
template <bool BX>
__global__ __launch_bounds__(256) void gemm_tn_batch_kernel(GemmTnBatch B) {
  int pi = 0;
  for (int i = 1; i < B.n; ++i)
    if ((int)blockIdx.x >= B.first[i]) pi = i;
  const GemmTnArgs& P = B.p[pi];
  const int rel = blockIdx.x - B.first[pi];   // (B.first[] are multiples of 8: a problem's workgroup `rel` runs on XCD rel % 8)
  const int gx = B.gx[pi], per = gx * B.gy[pi], gz = P.batch * P.taps * P.splits;
  if (rel >= per * gz) return;                 // padding up to the next problem's first workgroup
  int t, z;
  tn_xcd_order(rel, per, gz, P.xcd != 0, t, z);
  const int by = t / gx;
  gemm_tn_body<1, 1, true, true, BX>(P, t - by * gx, by, z);
}

__global__ void gemm_naive_kernel(ConvGemmProblem P) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)P.M * P.N) return;
  const int m = (int)(idx / P.N), n = (int)(idx % P.N);
  const int t = m % P.T;
  float acc = 0.f;
  for (int tap = 0; tap < P.taps; ++tap) {
    const int st = t + tap - P.pad_l;
    if (st < 0 || st >= P.T) continue;
    const float* a = P.A + (int64_t)(m + tap - P.pad_l) * P.lda;
    const float* w = P.W + (int64_t)tap * P.K * P.ldw + n;
    for (int k = 0; k < P.K; ++k) acc = fmaf(a[k], w[(int64_t)k * P.ldw], acc);
  }
  if (P.bias) acc += P.bias[n];
  P.C[(int64_t)m * P.ldc + n] = apply_act(acc, P.act);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

void conv_gemm_set_flags(ConvGemmProblem& p) {
  p.flags = 0;
  if (p.Nld <= 0) p.Nld = (p.N % 4 == 0) ? p.N : 0;   // loadable W columns (multiple of 4); 0 = no vector contract
  if (p.lda % 4 == 0 && aligned16(p.A) && p.K % 4 == 0) p.flags |= 1;
  if (p.ldw % 4 == 0 && aligned16(p.W) && ((int64_t)p.K * p.ldw) % 4 == 0 && p.Nld > 0 && p.Nld % 4 == 0 && p.Nld <= p.ldw)
    p.flags |= 2;
}

template <int WM, int WN>
static void dispatch_nn(int flags, dim3 grid, hipStream_t s, ConvGemmBatch& batch) {
  switch (flags & 3) {
    case 3: TACO_KLAUNCH((conv_gemm_kernel<WM, WN, true, true>), grid, dim3(256), 0, s, batch); break;
    case 1: TACO_KLAUNCH((conv_gemm_kernel<WM, WN, true, false>), grid, dim3(256), 0, s, batch); break;
    case 2: TACO_KLAUNCH((conv_gemm_kernel<WM, WN, false, true>), grid, dim3(256), 0, s, batch); break;
    default: TACO_KLAUNCH((conv_gemm_kernel<WM, WN, false, false>), grid, dim3(256), 0, s, batch); break;
  }
}

int launch_conv_gemm_batch(ConvGemmBatch& batch, hipStream_t stream) {
  TACO_REQUIRE(batch.n >= 1 && batch.n <= kMaxGemmBatch, "conv_gemm: batch size %d out of range", batch.n);
  int maxM = 0, maxN = 0, flags = 3;
  double work = 0;
  for (int i = 0; i < batch.n; ++i) {
    ConvGemmProblem& p = batch.p[i];
    TACO_REQUIRE(p.A && p.W && p.C, "conv_gemm: null operand");
    TACO_REQUIRE(p.M > 0 && p.N > 0 && p.K > 0 && p.taps > 0 && p.T > 0, "conv_gemm: bad dims M=%d N=%d K=%d taps=%d T=%d",
                 p.M, p.N, p.K, p.taps, p.T);
    TACO_REQUIRE(p.M % p.T == 0, "conv_gemm: M (%d) must be a multiple of T (%d)", p.M, p.T);
    conv_gemm_set_flags(p);
    flags &= p.flags;   // one kernel variant per launch: every problem of the batch must meet the contract
    maxM = p.M > maxM ? p.M : maxM;
    maxN = p.N > maxN ? p.N : maxN;
    work += (double)cdiv(p.M, 128) * cdiv(p.N, 128);
  }
  // pooled epilogue (ConvGemmProblem::pool) exists in gemm2.hip only: nothing is launched otherwise and the caller runs the
  // convolution and bn_maxpool as two passes
  bool any_pool = false;
  for (int i = 0; i < batch.n; ++i) any_pool = any_pool || batch.p[i].pool != 0;
  if (any_pool && !(flags == 3 && conv_gemm2_would_launch(batch))) return TACO_ENOTFOUND;
  double flops = 0;
  for (int i = 0; i < batch.n; ++i) flops += 2.0 * batch.p[i].M * batch.p[i].N * batch.p[i].K * batch.p[i].taps;
  const int pslot = taco_prof_begin(2, stream);
  {
    int tmax = 0, tmin = 1 << 30;
    for (int i = 0; i < batch.n; ++i) {
      tmax = std::max(tmax, batch.p[i].taps);
      tmin = std::min(tmin, batch.p[i].taps);
    }
    const ConvGemmProblem& q = batch.p[0];
    taco_prof_label(2, pslot, "nn n=%d M=%d N=%d K=%d taps=%d..%d%s%s%s%s%s", batch.n, q.M, q.N, q.K, tmin, tmax, q.pool ? (q.pool == 2 ? " pool2" : " pool1") : "",
                    q.keep ? " keep" : "", q.residual ? " res" : "", q.atomic_out ? " atomic" : "", q.bias_stride ? " rowbias" : "");
  }
  if (flags == 3) {
    // second-generation kernel (gemm2.hip: DMA-staged 32-deep k-tiles, 128 x 128 tiles) whenever the batch meets its
    // contract and has enough tiles to occupy the chip
    const int rc = launch_conv_gemm2(batch, stream);
    if (rc != TACO_ENOTFOUND) {
      taco_prof_end(2, pslot, stream, flops);
      if (rc != TACO_OK) return rc;
      TACO_LAUNCH_CHECK("conv_gemm2");
      return TACO_OK;
    }
  }
  TACO_REQUIRE(!any_pool, "conv_gemm: the pooled epilogue was promised by gemm2.hip and not delivered");
  // Big tiles only when they still fill the chip (256 CUs); otherwise 64x64 tiles for more workgroups.
  if (work >= 384) {
    dispatch_nn<2, 2>(flags, dim3(cdiv(maxM, 128), cdiv(maxN, 128), batch.n), stream, batch);
  } else {
    dispatch_nn<1, 1>(flags, dim3(cdiv(maxM, 64), cdiv(maxN, 64), batch.n), stream, batch);
  }
  taco_prof_end(2, pslot, stream, flops);
  TACO_LAUNCH_CHECK("conv_gemm");
  return TACO_OK;
}

// C = epilogue(slab_0 + ... + slab_{n-1}) for partial results written by the caller's own chunked launch (slabs: n x M x N floats,
// row pitch N); p describes the epilogue (bias / activation / affine / residual / C, ldc) and M, N, T.
int launch_conv_gemm_slab_sum(const ConvGemmProblem& p, const float* slabs, int n, hipStream_t stream) {
  TACO_REQUIRE(slabs && n >= 1 && p.M > 0 && p.N > 0 && p.N % 4 == 0 && p.C, "conv_gemm_slab_sum: bad arguments");
  const int64_t total4 = (int64_t)p.M * p.N / 4;
  const int grid = (int)((total4 + 255) / 256 > 2048 ? 2048 : (total4 + 255) / 256);
  TACO_KLAUNCH(conv_gemm_tapsum_kernel, dim3(grid), dim3(256), 0, stream, p, slabs, n);
  TACO_LAUNCH_CHECK("conv_gemm_slab_sum");
  return TACO_OK;
}

int launch_conv_gemm_tapsplit(const ConvGemmProblem& p, float* slabs, int64_t slab_floats, hipStream_t stream) {
  // Preferred: k-split on the second-generation kernel.  The (tap, 32-deep k-tile) sequence is cut into S chunks, each a
  // problem of ONE grouped gemm2 launch writing its own slab; S minimises a makespan model
  //   ceil(tiles * S / 256 CUs) * ceil(k-tiles / S)  +  slab round trip,
  // e.g. encoder proj1 (50 tiles x 192 k-tiles): S = 5 -> 250 workgroups of 39 k-tiles instead of 50 of 192.
  {
    ConvGemmProblem q = p;
    conv_gemm_set_flags(q);
    const int64_t mn = (int64_t)p.M * p.N;
    if (slabs && (q.flags & 3) == 3 && !p.atomic_out && p.N % 4 == 0 && gemm2_min_tiles() > 0 && mn > 0) {
      const int tiles = cdiv(p.M, 128) * cdiv(p.N, 128);
      const int nit = p.taps * cdiv(p.K, 32);
      int maxS = (int)std::min<int64_t>(std::min<int64_t>(kMaxGemmBatch, slab_floats / mn), nit / 6);
      int bestS = 1;
      double best = 1e30;
      for (int S = 1; S <= maxS; ++S) {
        const double slab_units = S > 1 ? (2.0 * S * mn * 4.0 / 4.0e12) / 1.7e-6 : 0.0;   // write + read at ~4 TB/s, in k-tile times
        const double cost = (double)cdiv((int64_t)tiles * S, 256) * cdiv(nit, S) + slab_units;
        if (cost < best * 0.97) {   // prefer fewer slabs unless the model gains >= 3 %
          best = cost;
          bestS = S;
        }
      }
      const int forced = sw_int<SW_KSPLIT>();   // tuning override
      if (forced >= 1 && forced <= maxS) bestS = forced;
      if (bestS >= 2) {
        ConvGemmBatch b;
        b.n = bestS;
        const int per = cdiv(nit, bestS);
        for (int c = 0; c < bestS; ++c) {
          ConvGemmProblem& r = b.p[c];
          r = ConvGemmProblem();
          r.A = p.A; r.lda = p.lda; r.W = p.W; r.ldw = p.ldw; r.Nld = p.Nld; r.C = slabs + c * mn; r.ldc = p.N;
          r.M = p.M; r.N = p.N; r.K = p.K; r.taps = p.taps; r.T = p.T; r.pad_l = p.pad_l; r.act = TACO_ACT_NONE;
          r.it0 = c * per;
          r.it1 = std::min(nit, (c + 1) * per);
          conv_gemm_set_flags(r);
        }
        const int pslot = taco_prof_begin(2, stream);
        taco_prof_label(2, pslot, "nn-ksplit S=%d M=%d N=%d K=%d taps=%d", bestS, p.M, p.N, p.K, p.taps);
        const int rc = launch_conv_gemm2(b, stream, /*force=*/true);
        if (rc == TACO_OK) {
          const int64_t total4 = mn / 4;
          const int grid = (int)((total4 + 255) / 256 > 2048 ? 2048 : (total4 + 255) / 256);
          TACO_KLAUNCH(conv_gemm_tapsum_kernel, dim3(grid), dim3(256), 0, stream, p, slabs, bestS);
          taco_prof_end(2, pslot, stream, 2.0 * p.M * p.N * p.K * p.taps);
          TACO_LAUNCH_CHECK("conv_gemm2 k-split");
          return TACO_OK;
        }
        taco_prof_cancel(2, pslot, stream);
        if (rc != TACO_ENOTFOUND) return rc;
      }
    }
  }
  const double tiles64 = (double)cdiv(p.M, 64) * cdiv(p.N, 64);
  // worth it only while the 64x64 grid leaves CUs idle (encoder proj1: 200 tiles, 241 -> 163 + 12 us; the post-net's 720 tiles
  // are better off unsplit), and every tap still has a deep K loop
  if (!slabs || p.taps < 2 || p.taps > kMaxGemmBatch || p.N % 4 != 0 || p.atomic_out || tiles64 > 320 || p.K < 512)
    return launch_conv_gemm(p, stream);
  ConvGemmBatch b;
  b.n = p.taps;
  const int64_t slab = (int64_t)p.M * p.N;
  for (int t = 0; t < p.taps; ++t) {
    ConvGemmProblem q;
    q.A = p.A; q.lda = p.lda; q.W = p.W + (int64_t)t * p.K * p.ldw; q.ldw = p.ldw; q.Nld = p.Nld;
    q.C = slabs + t * slab; q.ldc = p.N;
    q.M = p.M; q.N = p.N; q.K = p.K; q.taps = 1; q.T = p.T; q.pad_l = p.pad_l - t;   // row shift of tap t: t - pad_l
    q.act = TACO_ACT_NONE;
    b.p[t] = q;
  }
  TACO_TRY(launch_conv_gemm_batch(b, stream));
  const int64_t total4 = slab / 4;
  const int grid = (int)((total4 + 255) / 256 > 2048 ? 2048 : (total4 + 255) / 256);
  TACO_KLAUNCH(conv_gemm_tapsum_kernel, dim3(grid), dim3(256), 0, stream, p, slabs, p.taps);
  TACO_LAUNCH_CHECK("conv_gemm_tapsum");
  return TACO_OK;
}

int launch_conv_gemm(const ConvGemmProblem& p, hipStream_t stream) {
  ConvGemmBatch b;
  b.n = 1;
  b.p[0] = p;
  return launch_conv_gemm_batch(b, stream);
}

template <int WM, int WN>
static void dispatch_tn(int flags, dim3 grid, hipStream_t s, const GemmTnArgs& a) {
  switch (flags & 3) {
    case 3:
      // (bf16x3 only for row ranges inside the chain bound, bf16x3.h bf16x_max_chain: TACO_DETERMINISTIC=1's single-workgroup row ranges are not)
      if (env_bf16x() && a.chunk <= bf16x_max_chain()) TACO_KLAUNCH((gemm_tn_kernel<WM, WN, true, true, true>), grid, dim3(256), 0, s, a);
      else TACO_KLAUNCH((gemm_tn_kernel<WM, WN, true, true>), grid, dim3(256), 0, s, a);
      break;
    case 1: TACO_KLAUNCH((gemm_tn_kernel<WM, WN, true, false>), grid, dim3(256), 0, s, a); break;
    case 2: TACO_KLAUNCH((gemm_tn_kernel<WM, WN, false, true>), grid, dim3(256), 0, s, a); break;
    default: TACO_KLAUNCH((gemm_tn_kernel<WM, WN, false, false>), grid, dim3(256), 0, s, a); break;
  }
}

// Workgroups a weight-gradient launch aims for (TACO_TN_BLOCKS overrides; swept on S1: 384 / 768 / 1536 / 3072 -> family 5.17 / 4.67 / 4.49 / 4.45 ms per step).
static int tn_block_target() {
  const int x = sw_int<SW_TN_BLOCKS>();
  return x > 0 ? x : 3072;
}

// Validates one problem, derives its vector flags and split plan.  Returns the tile size used (64 or 128).
// `group_tiles`: output tiles of the whole grouped launch this problem is part of (0: on its own): the row range is split so
// that the GROUP reaches the workgroup target, not every member by itself (a group of eight one-tile problems used to be cut
// into 64-row chunks: 4096 atomics per 4 k-steps).
static int plan_gemm_tn(GemmTnArgs& a, bool force_small, dim3& grid, int64_t group_tiles = 0) {
  a.flags = 0;
  if (a.Nld <= 0) a.Nld = (a.N % 4 == 0) ? a.N : 0;
  // (the vector paths address an operand with 32-bit byte offsets against one buffer descriptor: its extent must stay below 2 GiB)
  const int64_t lim31 = (int64_t)1 << 31;
  if (a.lda % 4 == 0 && aligned16(a.A) && a.strideA % 4 == 0 && a.K % 4 == 0 && ((int64_t)a.M + a.taps + 48) * a.lda * 4 < lim31)
    a.flags |= 1;
  if (a.ldy % 4 == 0 && aligned16(a.Y) && a.strideY % 4 == 0 && a.Nld > 0 && a.Nld % 4 == 0 && a.Nld <= a.ldy &&
      ((int64_t)a.M + 16) * a.ldy * 4 < lim31)
    a.flags |= 2;
  // taps merged into K where K is no multiple of the 64-row tile (kernels.h GemmTnArgs::ktap; vector A operand only; |shift| <= 16)
  const bool merge_taps = sw_on<SW_TN_MERGE_TAPS>();   // (0: one tile row per tap, rounds 1-6; a test covers both)
  if (merge_taps && a.ktap == 0 && (a.flags & 1) && a.taps > 1 && a.taps <= 17 && a.K % 64 != 0 && a.pad_l <= 16 && a.taps - 1 - a.pad_l <= 16) {
    a.ktap = a.K;
    a.K *= a.taps;
    a.taps = 1;
  }
  // TACO_TN_BM=64|128 forces the tile (tuning harness); TACO_TN_BIG_TILES = least number of 128 x 128 tiles for the big tile
  const int force_bm = sw_int<SW_TN_BM>(), big_tiles = sw_int<SW_TN_BIG_TILES>();
  bool big = !force_small && (int64_t)cdiv(a.K, 128) * cdiv(a.N, 128) * a.taps * a.batch >= big_tiles && a.K >= 128 && a.N >= 128;
  if (!force_small && force_bm == 128 && a.K >= 128 && a.N >= 128) big = true;
  if (force_bm == 64) big = false;
  const int bm = big ? 128 : 64;
  const int64_t tiles = (int64_t)cdiv(a.K, bm) * cdiv(a.N, bm) * a.taps * a.batch;
  const int64_t fill = group_tiles > tiles ? group_tiles : tiles;
  int splits = taco_deterministic() ? 1 : (int)((tn_block_target() + fill - 1) / fill);   // deterministic: one workgroup owns the whole row range
  // at least 20 tiles of 16 rows per workgroup on the long row ranges: a 64 x 64 epilogue is 4096 atomics, and with the loads
  // as cheap as they are now short row ranges spend more time in it than in their MFMAs (profiles/r04_tn_lab.txt: no-atomics
  // build -35..-45 % on the launches that used to be cut into 64-100-row pieces; TACO_TN_BLOCKS sweep in the same file)
  const int max_splits = a.M >= 1280 ? cdiv(a.M, 320) : cdiv(a.M, 64);
  if (splits > max_splits) splits = max_splits;
  if (splits < 1) splits = 1;
  int chunk = cdiv(a.M, splits);
  chunk = cdiv(chunk, BK) * BK;
  splits = cdiv(a.M, chunk);
  a.splits = splits;
  a.chunk = chunk;
  grid = dim3(cdiv(a.K, bm), cdiv(a.N, bm), a.batch * a.taps * splits);
  a.xcd = sw_int<SW_TN_XCD>();   // XCD-aware block order (0: plain); a test covers both orders
  return bm;
}

int launch_gemm_tn(GemmTnArgs a, bool zero_first, hipStream_t stream) {
  TACO_REQUIRE(a.A && a.Y && a.W, "gemm_tn: null operand");
  TACO_REQUIRE(a.M > 0 && a.N > 0 && a.K > 0 && a.taps > 0 && a.T > 0 && a.batch > 0, "gemm_tn: bad dims");
  TACO_REQUIRE(a.M % a.T == 0, "gemm_tn: M (%d) must be a multiple of T (%d)", a.M, a.T);
  if (zero_first) {
    for (int b = 0; b < a.batch; ++b) {
      hipError_t e = hipMemset2DAsync(a.W + (int64_t)b * a.strideW, (size_t)a.ldw * 4, 0, (size_t)a.N * 4,
                                      (size_t)a.taps * a.K, stream);
      if (e != hipSuccess) {
        taco_set_error("gemm_tn memset: %s", hipGetErrorString(e));
        return TACO_ELAUNCH;
      }
    }
  }
  if (gemm_tn2_eligible(a)) {
    const int pslot2 = taco_prof_begin(2, stream);
    TACO_TRY(launch_gemm_tn2(&a, 1, stream));
    taco_prof_end(2, pslot2, stream, 2.0 * a.M * a.N * a.K * a.taps);
    TACO_LAUNCH_CHECK("gemm_tn2");
    return TACO_OK;
  }
  dim3 grid;
  const int bm = plan_gemm_tn(a, false, grid);
  const int pslot = taco_prof_begin(2, stream);
  taco_prof_label(2, pslot, "tn M=%d N=%d K=%d taps=%d batch=%d splits=%d bm=%d", a.M, a.N, a.K, a.taps, a.batch, a.splits, bm);
  if (bm == 128)
    dispatch_tn<2, 2>(a.flags, grid, stream, a);
  else
    dispatch_tn<1, 1>(a.flags, grid, stream, a);
  taco_prof_end(2, pslot, stream, 2.0 * a.M * a.N * a.K * a.taps * a.batch);
  TACO_LAUNCH_CHECK("gemm_tn");
  return TACO_OK;
}

// Accumulating (never zeroing) grouped launch.  Problems that do not meet the vector contract, or that are large enough
// for the 128x128 tile, are launched on their own.
int launch_gemm_tn_batch(GemmTnBatch& b, hipStream_t stream) {
  TACO_REQUIRE(b.n >= 0 && b.n <= kMaxTnBatch, "gemm_tn_batch: %d problems out of range", b.n);
  GemmTnBatch grouped;
  int blocks = 0;
  GemmTnArgs big[kMaxTnBatch];
  int nbig = 0;
  double big_flops = 0;
  int64_t group_tiles = 0;
  for (int i = 0; i < b.n; ++i) {
    dim3 grid;
    GemmTnArgs probe = b.p[i];
    if (probe.A && probe.M > 0 && probe.N > 0 && probe.K > 0 && probe.taps > 0 && probe.batch > 0 && !gemm_tn2_eligible(probe) &&
        plan_gemm_tn(probe, false, grid) == 64 && probe.flags == 3)
      group_tiles += (int64_t)grid.x * grid.y * probe.taps * probe.batch;
  }
  for (int i = 0; i < b.n; ++i) {
    GemmTnArgs a = b.p[i];
    TACO_REQUIRE(a.A && a.Y && a.W, "gemm_tn_batch: null operand");
    TACO_REQUIRE(a.M > 0 && a.N > 0 && a.K > 0 && a.taps > 0 && a.T > 0 && a.batch > 0 && a.M % a.T == 0, "gemm_tn_batch: bad dims");
    if (gemm_tn2_eligible(a)) {   // second-generation kernel: all eligible problems of the group share ONE grid
      big[nbig++] = a;
      big_flops += 2.0 * a.M * a.N * a.K * a.taps;
      continue;
    }
    dim3 grid;
    GemmTnArgs probe = a;
    const int bm = plan_gemm_tn(probe, false, grid, group_tiles);
    if (bm == 128 || probe.flags != 3) {
      TACO_TRY(launch_gemm_tn(a, false, stream));
      continue;
    }
    const int j = grouped.n++;
    grouped.p[j] = probe;
    grouped.first[j] = blocks;
    grouped.gx[j] = (int)grid.x;
    grouped.gy[j] = (int)grid.y;
    blocks += (int)(grid.x * grid.y * grid.z);
    blocks = (blocks + 7) & ~7;   // every problem starts on XCD 0 (tn_xcd_order); the <= 7 padding workgroups return at once
  }
  if (nbig > 0) {
    const int pslot = taco_prof_begin(2, stream);
    TACO_TRY(launch_gemm_tn2(big, nbig, stream));
    taco_prof_end(2, pslot, stream, big_flops);
    TACO_LAUNCH_CHECK("gemm_tn2 batch");
  }
  if (grouped.n > 0) {
    double flops = 0;
    for (int i = 0; i < grouped.n; ++i)
      flops += 2.0 * grouped.p[i].M * grouped.p[i].N * grouped.p[i].K * grouped.p[i].taps * grouped.p[i].batch;
    const int pslot = taco_prof_begin(2, stream);
    taco_prof_label(2, pslot, "tn-batch n=%d blocks=%d first: M=%d N=%d K=%d taps=%d", grouped.n, blocks, grouped.p[0].M, grouped.p[0].N, grouped.p[0].K,
                    grouped.p[0].taps);
    int max_chunk = 0;
    for (int i = 0; i < grouped.n; ++i) max_chunk = grouped.p[i].chunk > max_chunk ? grouped.p[i].chunk : max_chunk;
    if (env_bf16x() && max_chunk <= bf16x_max_chain()) TACO_KLAUNCH(gemm_tn_batch_kernel<true>, dim3(blocks), dim3(256), 0, stream, grouped);
    else TACO_KLAUNCH(gemm_tn_batch_kernel<false>, dim3(blocks), dim3(256), 0, stream, grouped);
    taco_prof_end(2, pslot, stream, flops);
    TACO_LAUNCH_CHECK("gemm_tn_batch");
  }
  b.n = 0;
  return TACO_OK;
}

int launch_gemm_naive(const ConvGemmProblem& p, hipStream_t stream) {
  const int64_t n = (int64_t)p.M * p.N;
  TACO_KLAUNCH(gemm_naive_kernel, dim3(cdiv(n, 256)), dim3(256), 0, stream, p);
  TACO_LAUNCH_CHECK("gemm_naive");
  return TACO_OK;
}

// ---- debug doors (include/taco_hip.h "op-level debug doors of the GEMM forms"): the atomic K-problem batch, the row bias, the
//      grouped and the strided-batch weight gradient, each built as model.hip builds it ----

extern "C" int taco_debug_conv_gemm_batch_atomic(const float* dbank, int lda, const float* const* WT, const float* residual, int ldr,
                                                 float* dx_out, int ldc, int M, int T, int F, int K, int N, void* stream) {
  const char* who = "taco_debug_conv_gemm_batch_atomic";
  TACO_REQUIRE(M > 0 && M <= kDoorMaxRows, "%s: M must be in [1, 2^22], got %d", who, M);
  TACO_REQUIRE(T > 0 && M % T == 0, "%s: T must be positive and divide M = %d, got %d", who, M, T);
  TACO_REQUIRE(F >= 1 && F <= kMaxGemmBatch, "%s: F must be in [1, %d], got %d", who, kMaxGemmBatch, F);
  TACO_REQUIRE(N > 0 && N <= kDoorMaxCols, "%s: N must be in [1, 2^14], got %d", who, N);
  TACO_REQUIRE(K > 0 && K <= kDoorMaxCols, "%s: K must be in [1, 2^14], got %d", who, K);
  TACO_REQUIRE(lda >= F * K, "%s: lda must be >= F K = %d, got %d", who, F * K, lda);
  TACO_REQUIRE(ldc >= N, "%s: ldc must be >= N = %d, got %d", who, N, ldc);
  TACO_REQUIRE(!residual || ldr >= N, "%s: ldr must be >= N = %d, got %d", who, N, ldr);
  TACO_REQUIRE(WT, "%s: WT is null", who);
  DoorOperands o;
  o.in(dbank, door_span(M, (int64_t)F * K, lda), "dbank");
  for (int f = 1; f <= F; ++f) o.in(WT[f - 1], (size_t)f * K * N * sizeof(float), "WT[%d]", f - 1);
  o.in_opt(residual, door_span(M, N, ldr), "residual");
  o.out(dx_out, door_span(M, N, ldc), "dx_out");
  TACO_TRY(o.check(who));
  ConvGemmBatch batch;
  batch.n = F;
  for (int k = 1; k <= F; ++k) {   // cbhg_bwd's fall-back of the gather
    ConvGemmProblem& p = batch.p[F - k];
    p = ConvGemmProblem();
    p.A = dbank + (k - 1) * K; p.lda = lda; p.W = WT[k - 1]; p.ldw = N; p.C = dx_out; p.ldc = ldc; p.M = M; p.N = N;
    p.K = K; p.taps = k; p.T = T; p.pad_l = (k - 1) - (k - 1) / 2; p.act = TACO_ACT_NONE; p.atomic_out = 1;
    if (k == 1) {
      p.residual = residual;
      p.ldr = ldr;
    }
  }
  return launch_conv_gemm_batch(batch, as_stream(stream));
}

extern "C" int taco_debug_conv_gemm_rowbias(const float* A, int lda, const float* W, int ldw, const float* rowb, int bias_stride, float* C,
                                            int ldc, int M, int T, int N, int K, void* stream) {
  const char* who = "taco_debug_conv_gemm_rowbias";
  TACO_REQUIRE(M > 0 && M <= kDoorMaxRows, "%s: M must be in [1, 2^22], got %d", who, M);
  TACO_REQUIRE(T > 0 && M % T == 0, "%s: T must be positive and divide M = %d, got %d", who, M, T);
  TACO_REQUIRE(N > 0 && N <= kDoorMaxCols, "%s: N must be in [1, 2^14], got %d", who, N);
  TACO_REQUIRE(K > 0 && K <= kDoorMaxCols, "%s: K must be in [1, 2^14], got %d", who, K);
  TACO_REQUIRE(lda >= K, "%s: lda must be >= K = %d, got %d", who, K, lda);
  TACO_REQUIRE(ldw >= N, "%s: ldw must be >= N = %d, got %d", who, N, ldw);
  TACO_REQUIRE(ldc >= N, "%s: ldc must be >= N = %d, got %d", who, N, ldc);
  TACO_REQUIRE(bias_stride >= N, "%s: bias_stride must be >= N = %d, got %d", who, N, bias_stride);
  DoorOperands o;
  o.in(A, door_span(M, K, lda), "A");
  o.in(W, door_span(K, N, ldw), "W");
  o.in(rowb, door_span(M / T, N, bias_stride), "rowb");
  o.out(C, door_span(M, N, ldc), "C");
  TACO_TRY(o.check(who));
  ConvGemmProblem p;   // the speaker site: dense_problem(...) + T + bias_stride
  p.A = A; p.lda = lda; p.W = W; p.ldw = ldw; p.bias = rowb; p.C = C; p.ldc = ldc;
  p.M = M; p.N = N; p.K = K; p.taps = 1; p.pad_l = 0; p.act = TACO_ACT_NONE;
  p.T = T;
  p.bias_stride = bias_stride;
  return launch_conv_gemm(p, as_stream(stream));
}

extern "C" int taco_debug_gemm_tn_group(int n, const float* const* A, const int* lda, const float* const* Y, const int* ldy,
                                        float* const* W, const int* ldw, float* const* dbias, const int* M, const int* N, const int* K,
                                        const int* taps, const int* T, const int* pad_l, void* stream) {
  const char* who = "taco_debug_gemm_tn_group";
  TACO_REQUIRE(n >= 1 && n <= kMaxTnBatch, "%s: n must be in [1, %d], got %d", who, kMaxTnBatch, n);
  TACO_REQUIRE(A && lda && Y && ldy && W && ldw && M && N && K && taps && T && pad_l, "%s: a table is null", who);
  DoorOperands o;
  for (int i = 0; i < n; ++i) {
    TACO_REQUIRE(M[i] > 0 && M[i] <= kDoorMaxRows, "%s: M[%d] must be in [1, 2^22], got %d", who, i, M[i]);
    TACO_REQUIRE(T[i] > 0 && M[i] % T[i] == 0, "%s: T[%d] must be positive and divide M[%d] = %d, got %d", who, i, i, M[i], T[i]);
    TACO_REQUIRE(N[i] > 0 && N[i] <= kDoorMaxCols, "%s: N[%d] must be in [1, 2^14], got %d", who, i, N[i]);
    TACO_REQUIRE(K[i] > 0 && K[i] <= kDoorMaxCols, "%s: K[%d] must be in [1, 2^14], got %d", who, i, K[i]);
    TACO_REQUIRE(taps[i] >= 1 && taps[i] <= 64, "%s: taps[%d] must be in [1, 64], got %d", who, i, taps[i]);
    TACO_REQUIRE(pad_l[i] >= -64 && pad_l[i] <= 64, "%s: pad_l[%d] must be in [-64, 64], got %d", who, i, pad_l[i]);
    TACO_REQUIRE(lda[i] >= K[i], "%s: lda[%d] must be >= K = %d, got %d", who, i, K[i], lda[i]);
    TACO_REQUIRE(ldy[i] >= N[i], "%s: ldy[%d] must be >= N = %d, got %d", who, i, N[i], ldy[i]);
    TACO_REQUIRE(ldw[i] >= N[i], "%s: ldw[%d] must be >= N = %d, got %d", who, i, N[i], ldw[i]);
    o.in(A[i], door_span(M[i], K[i], lda[i]), "A[%d]", i);
    o.in(Y[i], door_span(M[i], N[i], ldy[i]), "Y[%d]", i);
    o.out(W[i], door_span((int64_t)taps[i] * K[i], N[i], ldw[i]), "W[%d]", i);
    if (dbias) o.out_opt(dbias[i], (size_t)N[i] * sizeof(float), "dbias[%d]", i);
  }
  TACO_TRY(o.check(who));
  GemmTnBatch b;
  for (int i = 0; i < n; ++i) {   // model.hip `tn` inside a TnGroup scope
    GemmTnArgs a;
    a.dbias = dbias ? dbias[i] : nullptr;
    a.A = A[i]; a.lda = lda[i]; a.Y = Y[i]; a.ldy = ldy[i]; a.W = W[i]; a.ldw = ldw[i]; a.M = M[i]; a.N = N[i]; a.K = K[i];
    a.taps = taps[i]; a.T = T[i]; a.pad_l = pad_l[i];
    b.p[b.n++] = a;
  }
  return launch_gemm_tn_batch(b, as_stream(stream));
}

extern "C" int taco_debug_gemm_tn_strided(const float* A, int lda, int64_t strideA, const float* Y, int ldy, int64_t strideY, float* W,
                                          int ldw, int64_t strideW, int M, int N, int K, int T, int pad_l, int batch, void* stream) {
  const char* who = "taco_debug_gemm_tn_strided";
  TACO_REQUIRE(M > 0 && M <= kDoorMaxRows, "%s: M must be in [1, 2^22], got %d", who, M);
  TACO_REQUIRE(T > 0 && M % T == 0, "%s: T must be positive and divide M = %d, got %d", who, M, T);
  TACO_REQUIRE(N > 0 && N <= kDoorMaxCols, "%s: N must be in [1, 2^14], got %d", who, N);
  TACO_REQUIRE(K > 0 && K <= kDoorMaxCols, "%s: K must be in [1, 2^14], got %d", who, K);
  TACO_REQUIRE(batch >= 1 && batch <= 4096, "%s: batch must be in [1, 4096], got %d", who, batch);
  TACO_REQUIRE(pad_l >= -64 && pad_l <= 64, "%s: pad_l must be in [-64, 64], got %d", who, pad_l);
  TACO_REQUIRE(lda >= K, "%s: lda must be >= K = %d, got %d", who, K, lda);
  TACO_REQUIRE(ldy >= N, "%s: ldy must be >= N = %d, got %d", who, N, ldy);
  TACO_REQUIRE(ldw >= N, "%s: ldw must be >= N = %d, got %d", who, N, ldw);
  const int64_t needA = (int64_t)(M - 1) * lda + K, needY = (int64_t)(M - 1) * ldy + N, needW = (int64_t)(K - 1) * ldw + N;
  TACO_REQUIRE(strideA >= needA, "%s: strideA must be >= (M - 1) lda + K = %lld, got %lld", who, (long long)needA, (long long)strideA);
  TACO_REQUIRE(strideY >= needY, "%s: strideY must be >= (M - 1) ldy + N = %lld, got %lld", who, (long long)needY, (long long)strideY);
  TACO_REQUIRE(strideW >= needW, "%s: strideW must be >= (K - 1) ldw + N = %lld, got %lld", who, (long long)needW, (long long)strideW);
  DoorOperands o;
  o.in(A, (size_t)((batch - 1) * strideA + needA) * sizeof(float), "A");
  o.in(Y, (size_t)((batch - 1) * strideY + needY) * sizeof(float), "Y");
  o.out(W, (size_t)((batch - 1) * strideW + needW) * sizeof(float), "W");
  TACO_TRY(o.check(who));
  GemmTnArgs a;   // the decoder's `d keys` product (model.hip, "attention memory")
  a.A = A; a.lda = lda; a.Y = Y; a.ldy = ldy; a.W = W; a.ldw = ldw;
  a.M = M; a.N = N; a.K = K; a.taps = 1; a.T = T; a.pad_l = pad_l; a.batch = batch;
  a.strideA = strideA; a.strideY = strideY; a.strideW = strideW;
  return launch_gemm_tn(a, false, as_stream(stream));
}
