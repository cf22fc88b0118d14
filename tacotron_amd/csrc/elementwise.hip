// elementwise.hip -- HBM-bound glue kernels of the Tacotron hot path: embedding gather/scatter (tacotron.py:111-114),
// BN-affine + max-pool (ops.py:64-71), highway blend (ops.py:46), activation/dropout derivatives, column reductions
// for bias / BN gradients, L1 loss + sign gradient (tacotron.py:158-160), weight transposes for the backward GEMMs,
// global-norm clip + TF-form Adam (tacotron.py:167-185), the Bernoulli mask generator, the stop rule over stored alignments and
// the per-utterance alignment scores.
// All are float4-vectorised where the layout allows, grid-stride, one pass over their tensors.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int kThreads = 256;
inline int grid_for(int64_t n_items, int per_block = kThreads, int cap = 4096) {
  int64_t g = (n_items + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (int)g;
}

// any block size, the wave sums added in sequence behind a leading barrier.  NOT vocoder.hip's block_sum4 (four waves, pairwise).
__device__ __forceinline__ float block_sum(float v, float* red /* >= 4 floats LDS */) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  float t = 0.f;
  const int nw = (blockDim.x + 63) >> 6;
  for (int i = 0; i < nw; ++i) t += red[i];
  return t;
}

__global__ void embedding_kernel(const float* __restrict__ table, const int32_t* __restrict__ ids,
                                 float* __restrict__ out, int64_t rows, int V, int width) {
  const int w4 = width / 4;
  const int64_t total = rows * w4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / w4;
    const int c4 = (int)(i % w4);
    int id = ids[row];
    id = id < 0 ? 0 : (id >= V ? V - 1 : id);
    reinterpret_cast<float4*>(out)[i] = reinterpret_cast<const float4*>(table + (int64_t)id * width)[c4];
  }
}

// dtable[v] += sum of the dout rows whose id is v.  Workgroup (v, segment) handles the rows of its segment: its threads first
// list the matching rows (each thread scans a contiguous run, a block-wide prefix sum keeps the list sorted), then four row
// lanes x 64 column quads add the listed rows (lane l takes list entries l, l+4, ...; the lanes are summed in a fixed order).
// One segment (deterministic mode): plain read-modify-write, reproducible.  Several: one atomicAdd per element and segment.
// (Padded text makes id 0 by far the most frequent row -- a single workgroup walking all of its rows was 0.5 ms.)
constexpr int kEmbSeg = 4096;   // rows listed per pass (LDS: 16 KB)
__global__ __launch_bounds__(256) void embedding_bwd_kernel(const float* __restrict__ dout, const int32_t* __restrict__ ids,
                                                            float* __restrict__ dtable, int64_t rows, int V, int width,
                                                            int64_t rows_per_seg) {
  __shared__ int list[kEmbSeg];
  __shared__ int cnt[256];
  __shared__ float4 red[3][64];
  const int v = blockIdx.x, tid = threadIdx.x, q0 = tid & 63, rl = tid >> 6;
  const int W4 = width >> 2;
  const int64_t seg0 = (int64_t)blockIdx.y * rows_per_seg;
  const int64_t seg1 = min(rows, seg0 + rows_per_seg);
  float4 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);   // column quads q0, q0+64, ... (width <= 1024)
  for (int64_t base = seg0; base < seg1; base += kEmbSeg) {
    const int seg = (int)min((int64_t)kEmbSeg, seg1 - base);
    const int per = (seg + 255) >> 8;
    const int r0 = min(seg, tid * per), r1 = min(seg, r0 + per);
    int c = 0;
    for (int r = r0; r < r1; ++r) {
      int id = ids[base + r];
      id = id < 0 ? 0 : (id >= V ? V - 1 : id);
      c += id == v;
    }
    cnt[tid] = c;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {   // inclusive scan
      const int x = tid >= off ? cnt[tid - off] : 0;
      __syncthreads();
      cnt[tid] += x;
      __syncthreads();
    }
    int o = cnt[tid] - c;
    const int total = cnt[255];
    for (int r = r0; r < r1; ++r) {
      int id = ids[base + r];
      id = id < 0 ? 0 : (id >= V ? V - 1 : id);
      if (id == v) list[o++] = r;
    }
    __syncthreads();
#pragma unroll 4
    for (int j = rl; j < total; j += 4) {
      const float4* src = reinterpret_cast<const float4*>(dout + (base + list[j]) * width);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (q0 + i * 64 < W4) {
          const float4 d = src[q0 + i * 64];
          acc[i].x += d.x; acc[i].y += d.y; acc[i].z += d.z; acc[i].w += d.w;
        }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i * 64 >= W4) break;
    if (rl > 0) red[rl - 1][q0] = acc[i];
    __syncthreads();
    if (rl == 0 && q0 + i * 64 < W4) {
      float4 t = acc[i];
      for (int l = 0; l < 3; ++l) { t.x += red[l][q0].x; t.y += red[l][q0].y; t.z += red[l][q0].z; t.w += red[l][q0].w; }
      float* dst = dtable + (int64_t)v * width + (q0 + i * 64) * 4;
      if (gridDim.y == 1) {
        dst[0] += t.x; dst[1] += t.y; dst[2] += t.z; dst[3] += t.w;
      } else {
        atomicAdd(dst + 0, t.x); atomicAdd(dst + 1, t.y); atomicAdd(dst + 2, t.z); atomicAdd(dst + 3, t.w);
      }
    }
    __syncthreads();
  }
}

__global__ void bn_maxpool_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                  const float* __restrict__ beta, float* __restrict__ y, int B, int T, int C) {
  const int C4 = C / 4;
  const int64_t total = (int64_t)B * T * C4;
  const float rs = 1.0f / sqrtf(1.0f + kBnEps);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % C4);
    const int64_t row = i / C4;
    const int t = (int)(row % T);
    const float4 g = reinterpret_cast<const float4*>(gamma)[c4];
    const float4 b = reinterpret_cast<const float4*>(beta)[c4];
    const float4 a = reinterpret_cast<const float4*>(x)[i];
    float4 z = make_float4(a.x * (g.x * rs) + b.x, a.y * (g.y * rs) + b.y, a.z * (g.z * rs) + b.z, a.w * (g.w * rs) + b.w);
    if (t + 1 < T) {
      const float4 a2 = reinterpret_cast<const float4*>(x)[i + C4];
      z.x = fmaxf(z.x, a2.x * (g.x * rs) + b.x);
      z.y = fmaxf(z.y, a2.y * (g.y * rs) + b.y);
      z.z = fmaxf(z.z, a2.z * (g.z * rs) + b.z);
      z.w = fmaxf(z.w, a2.w * (g.w * rs) + b.w);
    }
    reinterpret_cast<float4*>(y)[i] = z;
  }
}

// blockDim = (64 channel quads, 4 row lanes); grid = (C/256 ceil, row chunks).  A row lane walks a CONTIGUOUS run of rows, so
// the three pooled neighbours z[row-1], z[row], z[row+1] and dy[row-1] roll through registers: x and dy are read once.
// x is the ReLU output the affine was applied to (ops.py:64-66: relu -> batch_norm -> max_pool): the ReLU backward (x > 0)
// is applied to the stored gradient in the same pass.
__global__ void bn_maxpool_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                      const float* __restrict__ beta, const float* __restrict__ dy,
                                      float* __restrict__ dx, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                      int B, int T, int C, int rows_per_block) {
  const int C4 = C >> 2;
  const int c4 = blockIdx.x * 64 + threadIdx.x;
  const int64_t M = (int64_t)B * T;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < M ? r0 + rows_per_block : M;
  const int seg = (rows_per_block + 3) >> 2;
  const int64_t ra = r0 + (int64_t)threadIdx.y * seg;
  const int64_t rb = ra + seg < r1 ? ra + seg : r1;
  const float rs = 1.0f / sqrtf(1.0f + kBnEps);
  float ag[4] = {0.f, 0.f, 0.f, 0.f}, ab[4] = {0.f, 0.f, 0.f, 0.f};
  if (c4 < C4 && ra < rb) {
    const float4 g4 = reinterpret_cast<const float4*>(gamma)[c4];
    const float4 be4 = reinterpret_cast<const float4*>(beta)[c4];
    const float sc[4] = {g4.x * rs, g4.y * rs, g4.z * rs, g4.w * rs};
    const float be[4] = {be4.x, be4.y, be4.z, be4.w};
    const float4* X = reinterpret_cast<const float4*>(x) + c4;
    const float4* DY = reinterpret_cast<const float4*>(dy) + c4;
    float4* DX = reinterpret_cast<float4*>(dx) + c4;
    int t = (int)(ra % T);
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 xp = t > 0 ? X[(ra - 1) * C4] : zero4, dyp = t > 0 ? DY[(ra - 1) * C4] : zero4;
    float4 xc = X[ra * C4];
    for (int64_t row = ra; row < rb; ++row) {
      const bool last = t == T - 1, first = t == 0;
      const float4 xn = last ? zero4 : X[(row + 1) * C4];
      const float4 dyc = DY[row * C4];
      const float xpv[4] = {xp.x, xp.y, xp.z, xp.w}, xcv[4] = {xc.x, xc.y, xc.z, xc.w}, xnv[4] = {xn.x, xn.y, xn.z, xn.w};
      const float dpv[4] = {dyp.x, dyp.y, dyp.z, dyp.w}, dcv[4] = {dyc.x, dyc.y, dyc.z, dyc.w};
      float o[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float z = xcv[q] * sc[q] + be[q];
        float dz = 0.f;
        if (last || z >= xnv[q] * sc[q] + be[q]) dz = dcv[q];          // y[row] = max(z[row], z[row+1]) takes z[row] on ties
        if (!first && z > xpv[q] * sc[q] + be[q]) dz += dpv[q];        // y[row-1] takes z[row] only when strictly larger
        o[q] = xcv[q] > 0.f ? dz * sc[q] : 0.f;
        ag[q] += dz * xcv[q] * rs;
        ab[q] += dz;
      }
      DX[row * C4] = make_float4(o[0], o[1], o[2], o[3]);
      xp = xc; xc = xn; dyp = dyc;
      t = last ? 0 : t + 1;
      if (last && row + 1 < rb) xc = X[(row + 1) * C4];   // next sequence starts: its first row was not fetched as a neighbour
    }
  }
  __shared__ float red[2][4][256];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    red[0][threadIdx.y][threadIdx.x * 4 + q] = ag[q];
    red[1][threadIdx.y][threadIdx.x * 4 + q] = ab[q];
  }
  __syncthreads();
  const int tid = threadIdx.y * 64 + threadIdx.x;   // 256 threads <-> 256 channels of the block
  const int c = blockIdx.x * 256 + tid;
  if (c < C) {
    float g = 0.f, b2 = 0.f;
    for (int i = 0; i < 4; ++i) {
      g += red[0][i][tid];
      b2 += red[1][i][tid];
    }
    atomicAdd(&dgamma[c], g);
    atomicAdd(&dbeta[c], b2);
  }
}

__global__ void highway_combine_kernel(const float* __restrict__ th, const float* __restrict__ x,
                                       float* __restrict__ y, int64_t M) {
  const int64_t total = M * (kCb / 4);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / (kCb / 4);
    const int c4 = (int)(i % (kCb / 4));
    const float4 t = reinterpret_cast<const float4*>(th + row * 2 * kCb)[c4];
    const float4 h = reinterpret_cast<const float4*>(th + row * 2 * kCb + kCb)[c4];
    const float4 xv = reinterpret_cast<const float4*>(x)[i];
    float4 o;
    o.x = h.x * t.x + xv.x * (1.f - t.x);
    o.y = h.y * t.y + xv.y * (1.f - t.y);
    o.z = h.z * t.z + xv.z * (1.f - t.z);
    o.w = h.w * t.w + xv.w * (1.f - t.w);
    reinterpret_cast<float4*>(y)[i] = o;
  }
}

__global__ void highway_combine_bwd_kernel(const float* __restrict__ th, const float* __restrict__ x,
                                           const float* __restrict__ dy, float* __restrict__ dth,
                                           float* __restrict__ dx, int64_t M) {
  const int64_t total = M * kCb;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / kCb;
    const int c = (int)(i % kCb);
    const float t = th[row * 2 * kCb + c];
    const float h = th[row * 2 * kCb + kCb + c];
    const float g = dy[i];
    dth[row * 2 * kCb + c] = g * (h - x[i]) * t * (1.f - t);
    dth[row * 2 * kCb + kCb + c] = h > 0.f ? g * t : 0.f;
    dx[i] = g * (1.f - t);
  }
}

__global__ void act_bwd_kernel(const float* __restrict__ y, const float* __restrict__ dy,
                               const uint8_t* __restrict__ keep, float* __restrict__ dz, int64_t n, int act) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float yv = y[i];
    float g = dy[i];
    if (act == TACO_ACT_RELU) g = yv > 0.f ? g : 0.f;
    else if (act == TACO_ACT_SIGMOID) g = g * yv * (1.f - yv);
    else if (act == TACO_ACT_TANH) g = g * (1.f - yv * yv);
    if (keep) g = keep[i] ? g * 2.0f : 0.f;
    dz[i] = g;
  }
}

// blockDim = (64 cols, 4 row lanes); grid = (N/64 ceil, row chunks)
__global__ void affine_act_bwd_kernel(const float* __restrict__ pre, const float* __restrict__ gamma,
                                      const float* __restrict__ dy, float* __restrict__ dz, float* __restrict__ dgamma,
                                      float* __restrict__ dbeta, int64_t M, int N, int act, int rows_per_block) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < M ? r0 + rows_per_block : M;
  const float rs = 1.0f / sqrtf(1.0f + kBnEps);
  float ag = 0.f, ab = 0.f;
  if (c < N) {
    const float s = gamma[c] * rs;
#pragma unroll 4
    for (int64_t row = r0 + threadIdx.y; row < r1; row += 4) {
      const float g = dy[row * N + c];
      const float p = pre[row * N + c];
      ag += g * p * rs;
      ab += g;
      float d = g * s;
      if (act == TACO_ACT_RELU && !(p > 0.f)) d = 0.f;
      dz[row * N + c] = d;
    }
  }
  __shared__ float red[2][4][64];
  red[0][threadIdx.y][threadIdx.x] = ag;
  red[1][threadIdx.y][threadIdx.x] = ab;
  __syncthreads();
  if (threadIdx.y == 0 && c < N) {
    float g = 0.f, b = 0.f;
    for (int i = 0; i < 4; ++i) {
      g += red[0][i][threadIdx.x];
      b += red[1][i][threadIdx.x];
    }
    atomicAdd(&dgamma[c], g);
    atomicAdd(&dbeta[c], b);
  }
}


// grid = (N/64 ceil, B); block = (64, 4)
__global__ void colsum_batched_kernel(const float* __restrict__ x, int ld, float* __restrict__ out, int T, int N) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  const int b = blockIdx.y;
  float a = 0.f;
  if (c < N)
    for (int t = threadIdx.y; t < T; t += 4) a += x[((int64_t)b * T + t) * ld + c];
  __shared__ float red[4][64];
  red[threadIdx.y][threadIdx.x] = a;
  __syncthreads();
  if (threadIdx.y == 0 && c < N)
    out[(int64_t)b * N + c] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

__global__ void mask_rows_kernel(const float* __restrict__ x, const int32_t* __restrict__ len, float* __restrict__ y,
                                 int B, int T, int C) {
  const int C4 = C / 4;
  const int64_t total = (int64_t)B * T * C4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / C4;
    const int b = (int)(row / T), t = (int)(row % T);
    float4 v = reinterpret_cast<const float4*>(x)[i];
    if (t >= len[b]) v = make_float4(0.f, 0.f, 0.f, 0.f);
    reinterpret_cast<float4*>(y)[i] = v;
  }
}

// out[b,s,:] = x[b,s,:] - mean over s' < len[b] of x[b,s',:]   (rows s >= len[b]: 0).  One thread per column walks the rows in
// order (reproducible).  Used for the attention memory of the decoder backward: d alignments only matter up to a per-step
// constant (the softmax backward removes the alignment-weighted mean), and removing the rows' common component BEFORE the
// fold with Wx_c keeps the per-row rounding errors relative to what the softmax backward actually sees.
__global__ __launch_bounds__(256) void center_rows_kernel(const float* __restrict__ x, const int32_t* __restrict__ len,
                                                          float* __restrict__ out, int T, int C) {
  // block = 4 row lanes x 64 column quads (256 columns); grid = (C/256 ceil, B, 4 row quarters).  Every block forms the column
  // means of its sequence itself (lane l sums rows l, l+4, ...; the four lanes are added in a fixed order: reproducible) and
  // writes one quarter of the rows.
  __shared__ float4 red[3][64];
  const int b = blockIdx.y;
  const int q = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int c4 = blockIdx.x * 64 + q, C4 = C >> 2;
  const bool act = c4 < C4;
  int n = len[b];
  n = n < 1 ? 1 : (n > T ? T : n);
  const float4* xb = reinterpret_cast<const float4*>(x + (int64_t)b * T * C) + (act ? c4 : 0);
  float4* ob = reinterpret_cast<float4*>(out + (int64_t)b * T * C) + (act ? c4 : 0);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
  for (int s = rl; s < n; s += 4) {
    const float4 v = xb[(int64_t)s * C4];
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  if (rl > 0) red[rl - 1][q] = acc;
  __syncthreads();
  if (rl == 0) {
    for (int l = 0; l < 3; ++l) { acc.x += red[l][q].x; acc.y += red[l][q].y; acc.z += red[l][q].z; acc.w += red[l][q].w; }
    const float inv = 1.0f / (float)n;
    red[0][q] = make_float4(acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv);
  }
  __syncthreads();
  const float4 mean = red[0][q];
  if (!act) return;
  const int per = (T + gridDim.z - 1) / gridDim.z;
  const int s0 = blockIdx.z * per, s1 = min(T, s0 + per);
#pragma unroll 4
  for (int s = s0 + rl; s < s1; s += 4) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (s < n) {
      v = xb[(int64_t)s * C4];
      v.x -= mean.x; v.y -= mean.y; v.z -= mean.z; v.w -= mean.w;
    }
    ob[(int64_t)s * C4] = v;
  }
}

// g[r][c] = y[r][c] > 0 ? scale * g[r][c] : 0  (ReLU + dropout backward against the stored, already masked activation; both
// tensors are column blocks of wider records: row pitches ldg / ldy)
__global__ void mask_pos_kernel(float* __restrict__ g, int ldg, const float* __restrict__ y, int ldy, int64_t rows, int cols,
                                float scale) {
  const int64_t total = rows * cols;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cols;
    const int c = (int)(i - r * cols);
    const float v = g[r * ldg + c];
    g[r * ldg + c] = y[r * ldy + c] > 0.f ? scale * v : 0.f;
  }
}

__global__ void add_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ y, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    y[i] = a[i] + b[i];
}

__global__ __launch_bounds__(1024) void l1_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ grad, int ldg,
                          float* __restrict__ loss_slot, int64_t M, int N) {
  // one wave per row at a time: the row/column split of the padded gradient costs no division, and a wave's 64 lanes walk a
  // row in coalesced 256-byte pieces (N = 1025 rows are not 16-byte aligned, so the accesses stay scalar)
  __shared__ float red[16];
  float acc = 0.f;
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t m = wave0; m < M; m += nwaves) {
    const float* ar = a + m * N;
    const float* br = b + m * N;
    float* gr = grad ? grad + m * ldg : nullptr;
    // four 64-wide pieces at a time: all eight loads (clamped addresses instead of a branch around them), then the arithmetic,
    // then the stores -- a load issued behind a store would have to wait for that store's acknowledgement before its use
    for (int n0 = 0; n0 < ldg; n0 += 256) {
      float av[4], bv[4], g[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int n = n0 + 64 * u + lane;
        const int nn = n < N ? n : N - 1;
        av[u] = ar[nn];
        bv[u] = br[nn];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int n = n0 + 64 * u + lane;
        const float d = av[u] - bv[u];
        const bool in = n < N;
        acc += in ? fabsf(d) : 0.f;
        g[u] = in ? (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) : 0.f;
      }
      if (gr) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int n = n0 + 64 * u + lane;
          if (n < ldg) gr[n] = g[u];
        }
      }
    }
  }
  const float t = block_sum(acc, red);
  if (threadIdx.x == 0) loss_slot[blockIdx.x] = t;   // one partial per block; finish_loss adds them in block order
}

// loss[1], loss[2] = ordered sums of the two terms' block partials (kLossParts each, zero-padded by the l1 launches);
// loss[0] = their sum (tacotron.py:160).  `out` (nullable) receives a copy of the three values.  One block, no atomics:
// the loss is reproducible bit for bit.
__global__ void finish_loss_kernel(float* __restrict__ loss, const float* __restrict__ parts, float* __restrict__ out) {
  __shared__ float red[8];
  float a = 0.f, b = 0.f;
  for (int i = threadIdx.x; i < kLossParts; i += blockDim.x) {
    a += parts[i];
    b += parts[kLossParts + i];
  }
  a = block_sum(a, red);
  b = block_sum(b, red);
  if (threadIdx.x == 0) {
    loss[1] = a; loss[2] = b; loss[0] = a + b;
    if (out) { out[0] = a + b; out[1] = a; out[2] = b; }
  }
}

__global__ void transpose_batch_kernel(TransposeBatch b) {
  __shared__ float tile[32][33];
  const int t = blockIdx.x;
  int ji = 0;
  for (int i = 1; i < b.n; ++i)
    if (t >= b.j[i].tile0) ji = i;
  const TransposeJob& J = b.j[ji];
  int rel = t - J.tile0;
  const int tn = (J.N + 31) / 32, tk = (J.K + 31) / 32;
  const int tp = rel / (tn * tk);
  rel -= tp * tn * tk;
  const int by = rel / tn, bx = rel - by * tn;
  const float* src = J.in + (int64_t)(J.taps - 1 - tp) * J.K * J.N;
  float* dst = J.out + (int64_t)tp * J.K * J.N;
  const int n0 = bx * 32, k0 = by * 32;
  const int ldi = J.ldi ? J.ldi : J.N, ldo = J.ldo ? J.ldo : J.K;
  for (int j = threadIdx.y; j < 32; j += 8) {
    const int k = k0 + j, n = n0 + threadIdx.x;
    tile[j][threadIdx.x] = (k < J.K && n < J.N) ? src[(int64_t)k * ldi + n] : 0.f;
  }
  __syncthreads();
  for (int j = threadIdx.y; j < 32; j += 8) {
    const int n = n0 + j, k = k0 + threadIdx.x;
    if (n < J.N && k < J.K) dst[(int64_t)n * ldo + k] = tile[threadIdx.x][j];
  }
}

__global__ void sumsq_kernel(const float* __restrict__ x, int64_t n, float* __restrict__ out) {
  __shared__ float red[8];
  float acc = 0.f;
  const int64_t n4 = n / 4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  float a1 = 0.f, a2 = 0.f, a3 = 0.f;
  for (; i + 3 * stride < n4; i += 4 * stride) {   // four independent 16-byte loads in flight per thread
    const float4 v0 = reinterpret_cast<const float4*>(x)[i];
    const float4 v1 = reinterpret_cast<const float4*>(x)[i + stride];
    const float4 v2 = reinterpret_cast<const float4*>(x)[i + 2 * stride];
    const float4 v3 = reinterpret_cast<const float4*>(x)[i + 3 * stride];
    acc += v0.x * v0.x + v0.y * v0.y + v0.z * v0.z + v0.w * v0.w;
    a1 += v1.x * v1.x + v1.y * v1.y + v1.z * v1.z + v1.w * v1.w;
    a2 += v2.x * v2.x + v2.y * v2.y + v2.z * v2.z + v2.w * v2.w;
    a3 += v3.x * v3.x + v3.y * v3.y + v3.z * v3.z + v3.w * v3.w;
  }
  for (; i < n4; i += stride) {
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    acc += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  acc += (a1 + a2) + a3;
  if (blockIdx.x == 0 && threadIdx.x < (n - n4 * 4)) {
    const float v = x[n4 * 4 + threadIdx.x];
    acc += v * v;
  }
  const float t = block_sum(acc, red);
  if (threadIdx.x == 0) out[blockIdx.x] = t;   // one partial per block (kSumsqParts blocks): no atomics, no pre-zeroing
}

// Every block first adds the kSumsqParts partial sums of squares in the same fixed order (=> the same global norm in every
// block and on every run), then updates its slice.  `err` (nullable): the decoder kernels' error words; when either is set
// the gradients are garbage (a cluster exchange timed out), so the update is SKIPPED and gnorm_out reads -1.
__global__ void clip_adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                 float* __restrict__ v, int64_t n, float lr_t, float cap, const float* __restrict__ sumsq,
                                 float* __restrict__ gnorm_out, const int32_t* __restrict__ err) {
  __shared__ float red[8];
  if (err && (err[0] | err[1])) {
    if (gnorm_out && blockIdx.x == 0 && threadIdx.x == 0) gnorm_out[0] = -1.f;
    return;
  }
  float part = 0.f;
  for (int i = threadIdx.x; i < kSumsqParts; i += blockDim.x) part += sumsq[i];
  const float gn = sqrtf(block_sum(part, red));
  const float scale = cap > 0.f ? cap / fmaxf(gn, cap) : 1.0f;
  if (gnorm_out && blockIdx.x == 0 && threadIdx.x == 0) gnorm_out[0] = gn;
  const float b1 = 0.9f, b2 = 0.999f, eps = 1e-8f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float gi = g[i] * scale;
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    p[i] = p[i] - lr_t * mi / (sqrtf(vi) + eps);
  }
}

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
    if (frames) {
      const int64_t n = (int64_t)frames[b] * frames_per_unit;
      Fb = n < 0 ? 0 : (n > F ? F : (int)n);
    }
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
  int Fb = F;
  if (frames) {
    const int64_t n = (int64_t)frames[b] * frames_per_unit;
    Fb = n < 0 ? 0 : (n > F ? F : (int)n);
  }
  Fb = __builtin_amdgcn_readfirstlane(Fb);
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
//
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
  const int tile = (int)(blockIdx.x % (uint32_t)ntile), b = (int)(blockIdx.x / (uint32_t)ntile);
  int Fb = F, s = TACO_PITCH_ONE;
  if (frames) {
    const int64_t n = (int64_t)frames[b] * frames_per_unit;
    Fb = n < 0 ? 0 : (n > F ? F : (int)n);
  }
  if constexpr (!CURVE) {
    if (step_q) {
      s = step_q[b];
      s = s < TACO_PITCH_MIN_STEP ? TACO_PITCH_MIN_STEP : (s > TACO_PITCH_MAX_STEP ? TACO_PITCH_MAX_STEP : s);
    }
  }
  Fb = __builtin_amdgcn_readfirstlane(Fb);
  if constexpr (!CURVE) s = __builtin_amdgcn_readfirstlane(s);
  const int tid = threadIdx.x, lane = tid & 63, fl = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int f0 = tile * kPitchFrames, f = f0 + fl;
  const float* __restrict__ src = mag_t + (int64_t)b * C * F + f;    // (C F <= 1025 * 8192: the offsets below fit 32 bits)
  float* __restrict__ dst = out + (int64_t)b * C * F + f;
  const bool live = f < Fb, inside = f < F;
  bool plain;
  if constexpr (CURVE) {
    if (step_q && live) {   // (a frame behind F_b keeps ONE: its step is never read)
      s = step_q[(int64_t)b * F + f];
      s = s < TACO_PITCH_MIN_STEP ? TACO_PITCH_MIN_STEP : (s > TACO_PITCH_MAX_STEP ? TACO_PITCH_MAX_STEP : s);
    }
    plain = __ballot(live && s != TACO_PITCH_ONE) == 0;
  } else {
    plain = f0 >= Fb || s == TACO_PITCH_ONE;
  }
  if (plain) {   // (uniform) nothing to shift: zeros behind the row's end, the row's own bits in front of it
    for (int kb = 2 * wave + h; kb < C; kb += 2 * kPitchWaves * kPitchBatch) {   // (kPitchBatch loads in flight per thread)
      float m[kPitchBatch];
#pragma unroll
      for (int u = 0; u < kPitchBatch; ++u) {
        const int k = kb + 2 * kPitchWaves * u;
        m[u] = (live && k < C) ? src[k * F] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < kPitchBatch; ++u) {
        const int k = kb + 2 * kPitchWaves * u;
        if (inside && k < C) dst[k * F] = m[u];
      }
    }
    return;
  }
  const int N = 2 * (C - 1), mask = N - 1;
  for (int j = tid; j < N; j += 64 * kPitchWaves) tab[j] = cospif((float)(2 * j) / (float)N);   // (2 j / N is exact)
  __syncthreads();

  // ---- cepstrum ----
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
    const int k = 2 * wave + 2 * kPitchWaves * u + h;
    m[u] = (live && k < C) ? src[k * F] : 1.0f;
  }
  for (int k0 = 2 * wave; k0 < C; k0 += 8 * kPitchWaves) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = k0 + 8 * kPitchWaves + 2 * kPitchWaves * u + h;
      nx[u] = (live && k < C) ? src[k * F] : 1.0f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = k0 + 2 * kPitchWaves * u + h;   // (k >= C: m = 1, v = 0, and the table is read at some valid index)
      const float v = logf(fmaxf(m[u], TACO_PITCH_FLOOR)) * ((k == 0 || k == C - 1) ? 0.5f * wt : wt);
      c0p += v;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
        acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(tab[((32 * nb + 1 + fl) * k) & mask], v, acc[nb], 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) m[u] = nx[u];
  }
  float* part = env;                       // [wave][n - 1][f], then [wave][h][f] for c[0]
  float* part0 = env + kPitchWaves * NR * kPitchFrames;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      part[((wave * NR) + 32 * nb + (r & 3) + 8 * (r >> 2) + 4 * h) * kPitchFrames + fl] = acc[nb][r];
  part0[(2 * wave + h) * kPitchFrames + fl] = c0p;
  __syncthreads();
  for (int e = tid; e < NR * kPitchFrames; e += 64 * kPitchWaves) {   // e = (n - 1) * 32 + f
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < kPitchWaves; ++w) t += part[w * NR * kPitchFrames + e];
    cep[kPitchFrames + e] = (e >> 5) < Q ? t : 0.f;   // the rectangular lifter
  }
  if (tid < kPitchFrames) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < 2 * kPitchWaves; ++w) t += part0[w * kPitchFrames + tid];
    cep[tid] = t;
  }
  __syncthreads();   // (nothing reads the partials from here on: env is the envelope's)

  // ---- envelope ----
  const float c0 = cep[fl];
  float cb[NB][16];   // 2 c[n][f], n = 32 nb + 1 + 2 j + h: this lane's B operands
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int j = 0; j < 16; ++j) cb[nb][j] = 2.0f * cep[(32 * nb + 1 + 2 * j + h) * kPitchFrames + fl];
  if (tid < kPitchFrames) {   // bin C - 1: cos(pi n) = (-1)^n
    float t = c0;
    for (int n = 1; n <= NR; ++n) {
      const float c2 = 2.0f * cep[n * kPitchFrames + tid];
      t += (n & 1) ? -c2 : c2;
    }
    env[(C - 1) * kPitchFrames + tid] = t;
  }
  const int nblk = (C - 1 + 31) >> 5;
  for (int kb = wave; kb < nblk; kb += kPitchWaves) {
    const int k = 32 * kb + fl;
    f32x16 d;
#pragma unroll
    for (int r = 0; r < 16; ++r) d[r] = c0;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int j = 0; j < 16; ++j)
        d = __builtin_amdgcn_mfma_f32_32x32x2f32(tab[((32 * nb + 1 + 2 * j + h) * k) & mask], cb[nb][j], d, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int kk = 32 * kb + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (kk < C - 1) env[kk * kPitchFrames + fl] = d[r];
    }
  }
  __syncthreads();

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
  const int tile = (int)(blockIdx.x % (uint32_t)ntile), b = (int)(blockIdx.x / (uint32_t)ntile);
  int Fb = F;
  if (frames) {
    const int64_t n = (int64_t)frames[b] * frames_per_unit;
    Fb = n < 0 ? 0 : (n > F ? F : (int)n);
  }
  Fb = __builtin_amdgcn_readfirstlane(Fb);
  const int tid = threadIdx.x, lane = tid & 63, fl = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pt = 2 * wave + h;   // = tid >> 5
  const int f0 = tile * kF0Frames, f = f0 + fl;
  const int L = lag_max - lag_min + 3;
  const bool live = f < Fb, inside = f < F;
  float* __restrict__ ac = acf ? acf + (int64_t)b * L * F + f : nullptr;   // (L F <= 512 * 8192: the offsets below fit 32 bits)
  if (f0 >= Fb) {   // (uniform) behind the row's end
    if (inside) {
      if (tid < kF0Frames) period[(int64_t)b * F + f] = strength[(int64_t)b * F + f] = 0.f;
      if (ac)
        for (int j = pt; j < L; j += kF0Parts) ac[j * F] = 0.f;
    }
    return;
  }
  const int N = 2 * (C - 1), mask = N - 1;
  for (int j = tid; j < N; j += 64 * kF0Waves) tab[j] = cospif((float)(2 * j) / (float)N);   // (2 j / N is exact)

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
// the squares around the mean), a thread's frames in ascending order and the threads' partials down a fixed tree.
__global__ __launch_bounds__(256) void f0_stats_kernel(const float* __restrict__ period, const float* __restrict__ other,
                                                       const int32_t* __restrict__ frames, int frames_per_unit,
                                                       float* __restrict__ stats, int F) {
  __shared__ float red[256];
  __shared__ int cnt[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  int Fb = F;
  if (frames) {
    const int64_t n = (int64_t)frames[b] * frames_per_unit;
    Fb = n < 0 ? 0 : (n > F ? F : (int)n);
  }
  const float* __restrict__ p = period + (int64_t)b * F;
  const float* __restrict__ o = other ? other + (int64_t)b * F : nullptr;
  float s = 0.f;
  int c = 0;
  for (int f = tid; f < Fb; f += 256) {
    const float pv = p[f], ov = o ? o[f] : 1.0f;
    if (pv > 0.f && ov > 0.f) {
      s += o ? log2f(ov) - log2f(pv) : log2f(pv);
      ++c;
    }
  }
  red[tid] = s;
  cnt[tid] = c;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
      red[tid] += red[tid + w];
      cnt[tid] += cnt[tid + w];
    }
    __syncthreads();
  }
  const int n = cnt[0];
  const float mean = n > 0 ? red[0] / (float)n : 0.f;
  __syncthreads();
  s = 0.f;
  for (int f = tid; f < Fb; f += 256) {
    const float pv = p[f], ov = o ? o[f] : 1.0f;
    if (pv > 0.f && ov > 0.f) {
      const float x = (o ? log2f(ov) - log2f(pv) : log2f(pv)) - mean;
      s += x * x;
    }
  }
  red[tid] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) {
    stats[3 * b] = (float)n;
    stats[3 * b + 1] = mean;
    stats[3 * b + 2] = n > 0 ? sqrtf(red[0] / (float)n) : 0.f;
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

// taco_corpus_batch: the forward map denorm_unframe_kernel inverts, fused into the batch gather.  out[b, e] =
// (float(src[index[b], e]) - mean[e % C]) / stdv[e % C] over rows of `row` = Td * C elements; T = _Float16 (the corpus as
// preprocess stores it) or float.  One IEEE subtraction and one correctly rounded division per element: the bits of NumPy's
// (x.astype(float32) - mean) / std.  V = elements per thread and access (the host picks the widest the base addresses and the row
// pitch allow: 16-byte loads of 8 halves with two 16-byte stores at best, scalar at worst).  A workgroup owns kCorpusU * 256 * V
// consecutive elements of one output row; a thread takes its column once (one modulo) and steps it by `step` = (256 V) % C with
// a compare, and walks its V elements with a compare each.  mean / stdv (16 KB at C = 2050) are read through the caches.
// A row whose index lies outside [0, N) reads nothing, is written as zeros and counted once in *n_bad.
constexpr int kCorpusU = 4;
template <typename T, int N>
struct alignas(sizeof(T) * N) CorpusVec {
  T v[N];
};
template <typename T, int V, bool STATS>
__global__ __launch_bounds__(256) void corpus_batch_kernel(const T* __restrict__ src, const int64_t* __restrict__ index,
                                                           const float* __restrict__ mean, const float* __restrict__ stdv,
                                                           float* __restrict__ out, int32_t* __restrict__ n_bad, int64_t N,
                                                           int64_t row, int C, int step, int chunks) {
  constexpr int VO = V < 4 ? V : 4;   // floats per store
  typedef CorpusVec<T, V> VIn;
  typedef CorpusVec<float, VO> VOut;
  const int b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;
  const int64_t i = index ? index[b] : (int64_t)b;
  const int64_t e0 = ((int64_t)chunk * (kCorpusU * 256) + threadIdx.x) * V;
  float* o = out + (int64_t)b * row;
  if (i < 0 || i >= N) {   // (uniform over the workgroup)
    if (n_bad && chunk == 0 && threadIdx.x == 0) atomicAdd(n_bad, 1);
    VOut z;
#pragma unroll
    for (int j = 0; j < VO; ++j) z.v[j] = 0.f;
#pragma unroll
    for (int u = 0; u < kCorpusU; ++u) {
      const int64_t e = e0 + (int64_t)u * 256 * V;
      if (e < row)
#pragma unroll
        for (int h = 0; h < V / VO; ++h) *reinterpret_cast<VOut*>(o + e + h * VO) = z;
    }
    return;
  }
  const T* s = src + i * row;
  VIn x[kCorpusU];
#pragma unroll
  for (int u = 0; u < kCorpusU; ++u) {   // all loads first; row % V == 0, so e < row covers the whole vector
    const int64_t e = e0 + (int64_t)u * 256 * V;
    if (e < row) x[u] = *reinterpret_cast<const VIn*>(s + e);
  }
  int col = 0;
  if (STATS) col = row <= 0x7fffffff ? (int)((uint32_t)e0 % (uint32_t)C) : (int)(e0 % C);
#pragma unroll
  for (int u = 0; u < kCorpusU; ++u) {
    const int64_t e = e0 + (int64_t)u * 256 * V;
    if (e < row) {
      float y[V];
      int c = col;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        y[j] = (float)x[u].v[j];
        if (STATS) {
          y[j] = (y[j] - mean[c]) / stdv[c];
          c = c + 1 == C ? 0 : c + 1;
        }
      }
#pragma unroll
      for (int h = 0; h < V / VO; ++h) {
        VOut w;
#pragma unroll
        for (int j = 0; j < VO; ++j) w.v[j] = y[h * VO + j];
        *reinterpret_cast<VOut*>(o + e + h * VO) = w;
      }
    }
    col += step;
    col = col >= C ? col - C : col;
  }
}

__global__ void bernoulli_kernel(uint8_t* __restrict__ out, int64_t n, uint32_t thresh, uint64_t seed) {
  // each thread produces 8 bytes from one 64-bit hash: 8-bit resolution per draw would be too coarse, so draw
  // one hash per byte pair (2 x 32-bit lanes).
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i * 2 < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t h = counter_hash(seed, (uint64_t)i);
    const uint32_t lo = (uint32_t)h, hi = (uint32_t)(h >> 32);
    out[i * 2] = lo < thresh ? 1 : 0;
    if (i * 2 + 1 < n) out[i * 2 + 1] = hi < thresh ? 1 : 0;
  }
}

// taco_infer_stop: rows t >= len[b] of one or two (B, Td, C) tensors become 0.  Grid-stride over (b, t) rows, one row per workgroup
// at a time; the rows that are kept are neither read nor written.
__global__ __launch_bounds__(256) void zero_tail_rows_kernel(float* __restrict__ x0, int C0, float* __restrict__ x1, int C1,
                                                             const int32_t* __restrict__ len, int B, int Td) {
  for (int row = blockIdx.x; row < B * Td; row += gridDim.x) {
    const int b = row / Td, t = row - b * Td;
    if (t < len[b]) continue;
    for (int c = threadIdx.x; c < C0; c += blockDim.x) x0[(int64_t)row * C0 + c] = 0.f;
    if (x1)
      for (int c = threadIdx.x; c < C1; c += blockDim.x) x1[(int64_t)row * C1 + c] = 0.f;
  }
}

// The end-detection rule of include/taco_hip.h (TacoStopRule) over stored alignments: one workgroup per batch row walks t in
// order.  a_t = first index of max_s alignments[b, t, s] over s < Tt (lowest index on ties: lane-local ascending scan, then a
// wave butterfly and a fixed-order pass over the four waves, all under the one total order (value desc, index asc)).
__global__ __launch_bounds__(256) void stop_rule_kernel(const float* __restrict__ align, const int32_t* __restrict__ text_length,
                                                        int32_t* __restrict__ len_out, int Tt, int Td, int end_offset, int hold,
                                                        int min_steps) {
  __shared__ float wv[4];
  __shared__ int wi[4];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int L = text_length[b];
  L = L < 1 ? 1 : (L > Tt ? Tt : L);
  const int target = L - 1 - end_offset > 0 ? L - 1 - end_offset : 0;
  int run = 0, len = Td;
  for (int t = 0; t < Td; ++t) {
    const float* al = align + ((int64_t)b * Td + t) * Tt;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int s = threadIdx.x; s < Tt; s += 256) {
      const float v = al[s];
      if (v > bv) bv = v, bi = s;
    }
    for (int o = 32; o; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
    }
    if (lane == 0) wv[wave] = bv, wi[wave] = bi;
    __syncthreads();
    bv = wv[0], bi = wi[0];
    for (int w = 1; w < 4; ++w)
      if (wv[w] > bv || (wv[w] == bv && wi[w] < bi)) bv = wv[w], bi = wi[w];
    __syncthreads();   // (wv / wi are rewritten in the next step)
    run = bi >= target ? run + 1 : 0;
    if (run >= hold && t + 1 >= min_steps) {   // (uniform: every thread holds the same run)
      len = min(Td, (t + 4) / 4 * 4);
      break;
    }
  }
  if (threadIdx.x == 0) len_out[b] = len;
}

// ---- alignment scores (include/taco_hip.h taco_alignment_scores) ------------------------------------------------------------------
// One workgroup of 16 waves per batch row, one launch, no workspace: the row's a_t record has to meet in one place for `back`,
// `skip` and `covered`, and 2 bytes per step fit the LDS of one workgroup, so nothing is handed from one workgroup to another.
// Unlike the stop rule there is no run counter: a step's (a_t, p_t, pad sum) depends on that step alone, so wave w takes the steps
// w, w + 16, ... on its own -- 64 lanes over Tt, 16-byte loads when Tt % 4 == 0 and the base is 16-byte aligned (every step then
// starts on a 16-byte boundary), 4-byte loads otherwise -- and the load of its next step is in flight while it reduces this one.
// The argmax is reduced on the DPP path under the total order (value desc, index asc): associative, commutative and idempotent, so
// the rotations of wave_max apply unchanged.  NaN elements never win a comparison; an all-NaN step keeps the sentinel index.
// Phase 2 walks the record 64 steps per wave with ballots and popcounts; `covered` is the popcount of an LDS bitmap that phase 1
// fills with ds_or (idempotent: no order dependence).  The two means are summed per wave in step order and over the waves in wave
// order: the same arguments give the same bits.
constexpr int kAlignWaves = 16;
constexpr int kAlignThreads = 64 * kAlignWaves;
constexpr int kAlignNone = 0x7fffffff;   // index of "no non-NaN element yet": loses every tie

template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ void argmax_dpp(float& bv, int& bi) {
  const float ov = dpp_move<CTRL, ROW_MASK>(bv, bv);   // (lanes outside the row mask and lanes without a source keep their own pair)
  const int oi = __builtin_amdgcn_update_dpp(bi, bi, CTRL, ROW_MASK, 0xf, false);
  if (ov > bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
}
__device__ __forceinline__ void wave_argmax(float& bv, int& bi) {
  argmax_dpp<0xb1>(bv, bi);          // quad_perm [1,0,3,2]
  argmax_dpp<0x4e>(bv, bi);          // quad_perm [2,3,0,1]
  argmax_dpp<0x124>(bv, bi);         // row_ror:4
  argmax_dpp<0x128>(bv, bi);         // row_ror:8
  argmax_dpp<0x142, 0xa>(bv, bi);    // row_bcast:15 -> rows 1,3
  argmax_dpp<0x143, 0xc>(bv, bi);    // row_bcast:31 -> rows 2,3
  bv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(bv), 63));
  bi = __builtin_amdgcn_readlane(bi, 63);
}
__device__ __forceinline__ void align_take(float v, int s, int L, float& bv, int& bi, float& pad) {
  if (v > bv || (v == bv && s < bi)) bv = v, bi = s;   // (both false for a NaN)
  if (s >= L) pad += v;
}
// item i of a step: VEC: elements 4 i .. 4 i + 3 in one 16-byte load; else element i
template <bool VEC>
__device__ __forceinline__ f32x4 align_load(const float* __restrict__ al, int i) {
  if (VEC) return *reinterpret_cast<const f32x4*>(al + 4 * i);
  f32x4 v = {al[i], 0.f, 0.f, 0.f};
  return v;
}
template <bool VEC>
__device__ __forceinline__ void align_scan(f32x4 v, int i, int L, float& bv, int& bi, float& pad) {
  if (VEC) {
    align_take(v.x, 4 * i, L, bv, bi, pad);
    align_take(v.y, 4 * i + 1, L, bv, bi, pad);
    align_take(v.z, 4 * i + 2, L, bv, bi, pad);
    align_take(v.w, 4 * i + 3, L, bv, bi, pad);
  } else {
    align_take(v.x, i, L, bv, bi, pad);
  }
}
__device__ __forceinline__ int wave_imax(int v) {
  for (int o = 32; o; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_isum(int v) {
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <bool VEC>
__global__ __launch_bounds__(kAlignThreads) void alignment_scores_kernel(const float* __restrict__ align,
                                                                         const int32_t* __restrict__ text_length,
                                                                         const int32_t* __restrict__ steps, int max_jump,
                                                                         int32_t* __restrict__ counts, float* __restrict__ means, int Td,
                                                                         int Tt) {
  __shared__ uint16_t rec[TACO_ALIGNMENT_MAX_TD];          // a_t of the scored steps
  __shared__ uint32_t seen[TACO_ALIGNMENT_MAX_TT / 32];    // bit s: a_t == s for some scored t (s < L only)
  __shared__ float wsum[kAlignWaves][2];
  __shared__ int wcnt[kAlignWaves][5];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int L = text_length[b];
  L = L < 1 ? 1 : (L > Tt ? Tt : L);
  int n = steps ? steps[b] : Td;
  n = n < 0 ? 0 : (n > Td ? Td : n);
  const int words = (L + 31) >> 5;
  for (int w = threadIdx.x; w < words; w += kAlignThreads) seen[w] = 0u;
  __syncthreads();

  // phase 1: a wave per step
  const float* row = align + (int64_t)b * Td * Tt;
  const int items = VEC ? Tt >> 2 : Tt;
  float fsum = 0.f, psum = 0.f;
  f32x4 cur = {0.f, 0.f, 0.f, 0.f};
  if (wave < n && lane < items) cur = align_load<VEC>(row + (int64_t)wave * Tt, lane);
  for (int t = wave; t < n; t += kAlignWaves) {   // (wave-uniform trip count: every lane reaches the DPP reductions)
    const float* al = row + (int64_t)t * Tt;
    f32x4 nxt = {0.f, 0.f, 0.f, 0.f};
    if (t + kAlignWaves < n && lane < items) nxt = align_load<VEC>(al + (int64_t)kAlignWaves * Tt, lane);
    float bv = -INFINITY, pad = 0.f;
    int bi = kAlignNone;
    if (lane < items) align_scan<VEC>(cur, lane, L, bv, bi, pad);
    for (int i = lane + 64; i < items; i += 64) align_scan<VEC>(align_load<VEC>(al, i), i, L, bv, bi, pad);
    wave_argmax(bv, bi);
    pad = wave_sum(pad);
    const bool none = bi == kAlignNone;                    // every element is NaN: a_t = 0 and p_t = a[t, 0], a NaN
    const int a = none ? 0 : bi;
    fsum += none ? __builtin_nanf("") : bv;
    psum += pad;
    if (lane == 0) {
      rec[t] = (uint16_t)a;
      if (a < L) atomicOr(&seen[a >> 5], 1u << (a & 31));
    }
    cur = nxt;
  }
  if (lane == 0) wsum[wave][0] = fsum, wsum[wave][1] = psum;
  __syncthreads();

  // phase 2: the record, 64 steps per wave and pass
  int end = 0, n_pad = 0, n_back = 0, n_skip = 0;
  for (int t0 = wave * 64; t0 < n; t0 += kAlignThreads) {
    const int t = t0 + lane;
    const bool in = t < n;
    const int a = in ? (int)rec[t] : 0;
    const int prev = in && t > 0 ? (int)rec[t - 1] : a;
    end = max(end, a);
    n_pad += __popcll(__ballot(in && a >= L));
    n_back += __popcll(__ballot(in && a < prev));
    n_skip += __popcll(__ballot(in && a - prev > max_jump));
  }
  end = wave_imax(end);
  int cov = 0;
  for (int w = threadIdx.x; w < words; w += kAlignThreads) cov += __popc(seen[w]);
  cov = wave_isum(cov);
  if (lane == 0) wcnt[wave][0] = end, wcnt[wave][1] = n_pad, wcnt[wave][2] = n_back, wcnt[wave][3] = n_skip, wcnt[wave][4] = cov;
  __syncthreads();
  if (threadIdx.x == 0) {
    int c[5] = {0, 0, 0, 0, 0};
    float f = 0.f, p = 0.f;
    for (int w = 0; w < kAlignWaves; ++w) {
      c[0] = max(c[0], wcnt[w][0]);
      for (int k = 1; k < 5; ++k) c[k] += wcnt[w][k];
      f += wsum[w][0];
      p += wsum[w][1];
    }
    int32_t* co = counts + (int64_t)b * 6;
    co[0] = n;
    for (int k = 0; k < 5; ++k) co[1 + k] = c[k];
    means[(int64_t)b * 2] = n ? f / (float)n : 0.f;
    means[(int64_t)b * 2 + 1] = n ? p / (float)n : 0.f;
  }
}

}  // namespace

#define EW_LAUNCH(kernel, n_items, stream, ...)                                                        \
  do {                                                                                                 \
    TACO_KLAUNCH(kernel, dim3(grid_for(n_items)), dim3(kThreads), 0, stream, __VA_ARGS__);      \
    TACO_LAUNCH_CHECK(#kernel);                                                                        \
  } while (0)

int launch_embedding(const float* table, const int32_t* ids, float* out, int64_t rows, int V, hipStream_t s, int width) {
  TACO_REQUIRE(width % 4 == 0, "embedding: width %% 4 != 0");
  EW_LAUNCH(embedding_kernel, rows * (width / 4), s, table, ids, out, rows, V, width);
  return TACO_OK;
}
int launch_embedding_bwd(const float* dout, const int32_t* ids, float* dtable, int64_t rows, int V, hipStream_t s, int width) {
  TACO_REQUIRE(width <= 1024 && width % 4 == 0, "embedding_bwd: width %d must be a multiple of 4, <= 1024", width);
  int segs = taco_deterministic() ? 1 : (int)std::min<int64_t>(32, (rows + 255) / 256);
  if (segs < 1) segs = 1;
  const int64_t rps = (rows + segs - 1) / segs;
  TACO_KLAUNCH(embedding_bwd_kernel, dim3(V, segs), dim3(256), 0, s, dout, ids, dtable, rows, V, width, rps);
  TACO_LAUNCH_CHECK("embedding_bwd");
  return TACO_OK;
}
int launch_center_rows(const float* x, const int32_t* len, float* out, int B, int T, int C, hipStream_t s) {
  TACO_REQUIRE(C % 4 == 0, "center_rows: C %% 4 != 0");
  TACO_KLAUNCH(center_rows_kernel, dim3((C + 255) / 256, B, 4), dim3(256), 0, s, x, len, out, T, C);
  TACO_LAUNCH_CHECK("center_rows");
  return TACO_OK;
}
int launch_mask_pos(float* g, int ldg, const float* y, int ldy, int64_t rows, int cols, float scale, hipStream_t s) {
  EW_LAUNCH(mask_pos_kernel, rows * cols, s, g, ldg, y, ldy, rows, cols, scale);
  return TACO_OK;
}
int launch_colsum_batched(const float* x, int ld, float* out, int B, int T, int N, hipStream_t s) {
  TACO_KLAUNCH(colsum_batched_kernel, dim3((N + 63) / 64, B), dim3(64, 4), 0, s, x, ld, out, T, N);
  TACO_LAUNCH_CHECK("colsum_batched");
  return TACO_OK;
}
// ---- debug doors of the glue kernels (include/taco_hip.h "op-level debug doors of the train step's glue kernels"): each checks its
//      arguments by name, calls the launch_* above it with the caller's stream and returns its code; no kernel of their own ----
#define DOOR_ROWS(who, name, v) TACO_REQUIRE((v) > 0 && (v) <= kDoorMaxRows, "%s: %s must be in [1, 2^22], got %lld", who, name, (long long)(v))
#define DOOR_COLS(who, name, v) TACO_REQUIRE((v) > 0 && (v) <= kDoorMaxCols, "%s: %s must be in [1, 2^14], got %lld", who, name, (long long)(v))
#define DOOR_COLS4(who, name, v) \
  TACO_REQUIRE((v) > 0 && (v) <= kDoorMaxCols && (v) % 4 == 0, "%s: %s must be a multiple of 4 in [4, 2^14], got %lld", who, name, (long long)(v))
#define DOOR_PITCH(who, name, v, least) TACO_REQUIRE((v) >= (least), "%s: %s must be >= %lld, got %lld", who, name, (long long)(least), (long long)(v))
constexpr int64_t kDoorMaxElems = (int64_t)1 << 31;   // flat element counts (act_bwd, add, sumsq)
extern "C" int taco_debug_embedding(const float* table, const int32_t* ids, float* out, int rows, int V, int width, void* stream) {
  const char* who = "taco_debug_embedding";
  DOOR_ROWS(who, "rows", rows);
  DOOR_COLS(who, "V", V);
  DOOR_COLS4(who, "width", width);
  DoorOperands o;
  o.in(table, (size_t)V * width * sizeof(float), "table");
  o.in(ids, (size_t)rows * sizeof(int32_t), "ids");
  o.out(out, (size_t)rows * width * sizeof(float), "out");
  TACO_TRY(o.check(who));
  return launch_embedding(table, ids, out, rows, V, as_stream(stream), width);
}
extern "C" int taco_debug_embedding_bwd(const float* dout, const int32_t* ids, float* dtable, int rows, int V, int width, void* stream) {
  const char* who = "taco_debug_embedding_bwd";
  DOOR_ROWS(who, "rows", rows);
  DOOR_COLS(who, "V", V);
  TACO_REQUIRE(width > 0 && width <= 1024 && width % 4 == 0, "%s: width must be a multiple of 4 in [4, 1024], got %d", who, width);
  DoorOperands o;
  o.in(dout, (size_t)rows * width * sizeof(float), "dout");
  o.in(ids, (size_t)rows * sizeof(int32_t), "ids");
  o.out(dtable, (size_t)V * width * sizeof(float), "dtable");
  TACO_TRY(o.check(who));
  return launch_embedding_bwd(dout, ids, dtable, rows, V, as_stream(stream), width);
}
extern "C" int taco_debug_center_rows(const float* x, const int32_t* len, float* out, int B, int T, int C, void* stream) {
  const char* who = "taco_debug_center_rows";
  TACO_REQUIRE(B > 0 && B <= 65535 && T > 0 && (int64_t)B * T <= kDoorMaxRows, "%s: B must be in [1, 65535] and B T in [1, 2^22], got B = %d, T = %d", who, B, T);
  DOOR_COLS4(who, "C", C);
  const size_t mc = (size_t)B * T * C * sizeof(float);
  DoorOperands o;
  o.in(x, mc, "x");
  o.in(len, (size_t)B * sizeof(int32_t), "len");
  o.out(out, mc, "out");
  TACO_TRY(o.check(who));
  return launch_center_rows(x, len, out, B, T, C, as_stream(stream));
}
extern "C" int taco_debug_mask_pos(float* g, int ldg, const float* y, int ldy, int rows, int cols, float scale, void* stream) {
  const char* who = "taco_debug_mask_pos";
  DOOR_ROWS(who, "rows", rows);
  DOOR_COLS(who, "cols", cols);
  DOOR_PITCH(who, "ldg", ldg, cols);
  DOOR_PITCH(who, "ldy", ldy, cols);
  DoorOperands o;
  o.out(g, door_span(rows, cols, ldg), "g");
  o.in(y, door_span(rows, cols, ldy), "y");
  TACO_TRY(o.check(who));
  return launch_mask_pos(g, ldg, y, ldy, rows, cols, scale, as_stream(stream));
}
extern "C" int taco_debug_colsum_batched(const float* x, int ld, float* out, int B, int T, int N, void* stream) {
  const char* who = "taco_debug_colsum_batched";
  TACO_REQUIRE(B > 0 && B <= 65535 && T > 0 && (int64_t)B * T <= kDoorMaxRows, "%s: B must be in [1, 65535] and B T in [1, 2^22], got B = %d, T = %d", who, B, T);
  DOOR_COLS(who, "N", N);
  DOOR_PITCH(who, "ld", ld, N);
  DoorOperands o;
  o.in(x, door_span((int64_t)B * T, N, ld), "x");
  o.out(out, (size_t)B * N * sizeof(float), "out");
  TACO_TRY(o.check(who));
  return launch_colsum_batched(x, ld, out, B, T, N, as_stream(stream));
}
int launch_bn_maxpool(const float* x, const float* gamma, const float* beta, float* y, int B, int T, int C, hipStream_t s) {
  TACO_REQUIRE(C % 4 == 0, "bn_maxpool: C %% 4 != 0");
  EW_LAUNCH(bn_maxpool_kernel, (int64_t)B * T * (C / 4), s, x, gamma, beta, y, B, T, C);
  return TACO_OK;
}
static inline void col_grid(int64_t M, int N, dim3& grid, int& rpb) {
  int chunks = (int)((M + 31) / 32);   // 8 rows per thread: enough blocks to cover 256 CUs even for 128-column tensors
  if (chunks > 2048) chunks = 2048;
  if (taco_deterministic()) chunks = 1;   // one workgroup per column range sums all rows in a fixed order: a single atomicAdd each
  if (chunks < 1) chunks = 1;
  rpb = (int)((M + chunks - 1) / chunks);
  grid = dim3((N + 63) / 64, (unsigned)((M + rpb - 1) / rpb));
}
int launch_bn_maxpool_bwd(const float* x, const float* gamma, const float* beta, const float* dy, float* dx,
                          float* dgamma, float* dbeta, int B, int T, int C, hipStream_t s) {
  dim3 grid;
  int rpb;
  TACO_REQUIRE(C % 4 == 0, "bn_maxpool_bwd: C %% 4 != 0");
  col_grid((int64_t)B * T, C, grid, rpb);
  grid.x = (C / 4 + 63) / 64;
  TACO_KLAUNCH(bn_maxpool_bwd_kernel, grid, dim3(64, 4), 0, s, x, gamma, beta, dy, dx, dgamma, dbeta, B, T, C, rpb);
  TACO_LAUNCH_CHECK("bn_maxpool_bwd");
  return TACO_OK;
}
// ---- debug doors (include/taco_hip.h "op-level debug doors of the GEMM forms"): the two-pass twins of the pooled epilogues ----
extern "C" int taco_debug_bn_maxpool_fwd(const float* x, const float* gamma, const float* beta, float* y, int B, int T, int C, void* stream) {
  const char* who = "taco_debug_bn_maxpool_fwd";
  TACO_REQUIRE(B > 0 && T > 0 && (int64_t)B * T <= kDoorMaxRows, "%s: B T must be in [1, 2^22], got B = %d, T = %d", who, B, T);
  TACO_REQUIRE(C > 0 && C <= kDoorMaxCols && C % 4 == 0, "%s: C must be a multiple of 4 in [4, 2^14], got %d", who, C);
  const size_t mc = (size_t)B * T * C * sizeof(float);
  DoorOperands o;
  o.in(x, mc, "x");
  o.in(gamma, (size_t)C * sizeof(float), "gamma");
  o.in(beta, (size_t)C * sizeof(float), "beta");
  o.out(y, mc, "y");
  TACO_TRY(o.check(who));
  return launch_bn_maxpool(x, gamma, beta, y, B, T, C, as_stream(stream));
}
extern "C" int taco_debug_bn_maxpool_bwd(const float* x, const float* gamma, const float* beta, const float* dy, float* dx, float* dgamma,
                                         float* dbeta, int B, int T, int C, void* stream) {
  const char* who = "taco_debug_bn_maxpool_bwd";
  TACO_REQUIRE(B > 0 && T > 0 && (int64_t)B * T <= kDoorMaxRows, "%s: B T must be in [1, 2^22], got B = %d, T = %d", who, B, T);
  TACO_REQUIRE(C > 0 && C <= kDoorMaxCols && C % 4 == 0, "%s: C must be a multiple of 4 in [4, 2^14], got %d", who, C);
  const size_t mc = (size_t)B * T * C * sizeof(float);
  DoorOperands o;
  o.in(x, mc, "x");
  o.in(gamma, (size_t)C * sizeof(float), "gamma");
  o.in(beta, (size_t)C * sizeof(float), "beta");
  o.in(dy, mc, "dy");
  o.out(dx, mc, "dx");
  o.out(dgamma, (size_t)C * sizeof(float), "dgamma");
  o.out(dbeta, (size_t)C * sizeof(float), "dbeta");
  TACO_TRY(o.check(who));
  return launch_bn_maxpool_bwd(x, gamma, beta, dy, dx, dgamma, dbeta, B, T, C, as_stream(stream));
}
int launch_highway_combine(const float* th, const float* x, float* y, int64_t M, hipStream_t s) {
  EW_LAUNCH(highway_combine_kernel, M * (kCb / 4), s, th, x, y, M);
  return TACO_OK;
}
int launch_highway_combine_bwd(const float* th, const float* x, const float* dy, float* dth, float* dx, int64_t M,
                               hipStream_t s) {
  EW_LAUNCH(highway_combine_bwd_kernel, M * kCb, s, th, x, dy, dth, dx, M);
  return TACO_OK;
}
int launch_act_bwd(const float* y, const float* dy, const uint8_t* keep, float* dz, int64_t n, int act, hipStream_t s) {
  EW_LAUNCH(act_bwd_kernel, n, s, y, dy, keep, dz, n, act);
  return TACO_OK;
}
int launch_affine_act_bwd(const float* pre, const float* gamma, const float* dy, float* dz, float* dgamma, float* dbeta,
                          int64_t M, int N, int act, hipStream_t s) {
  dim3 grid;
  int rpb;
  col_grid(M, N, grid, rpb);
  TACO_KLAUNCH(affine_act_bwd_kernel, grid, dim3(64, 4), 0, s, pre, gamma, dy, dz, dgamma, dbeta, M, N, act, rpb);
  TACO_LAUNCH_CHECK("affine_act_bwd");
  return TACO_OK;
}
int launch_mask_rows(const float* x, const int32_t* len, float* y, int B, int T, int C, hipStream_t s) {
  TACO_REQUIRE(C % 4 == 0, "mask_rows: C %% 4 != 0");
  EW_LAUNCH(mask_rows_kernel, (int64_t)B * T * (C / 4), s, x, len, y, B, T, C);
  return TACO_OK;
}
int launch_zero_tail_rows(float* x0, int C0, float* x1, int C1, const int32_t* len, int B, int Td, hipStream_t s) {
  const int rows = B * Td;
  TACO_KLAUNCH(zero_tail_rows_kernel, dim3(rows < 4096 ? rows : 4096), dim3(256), 0, s, x0, C0, x1, C1, len, B, Td);
  TACO_LAUNCH_CHECK("zero_tail_rows");
  return TACO_OK;
}
extern "C" int taco_debug_highway_combine(const float* th, const float* x, float* y, int M, void* stream) {
  const char* who = "taco_debug_highway_combine";
  DOOR_ROWS(who, "M", M);
  DoorOperands o;
  o.in(th, (size_t)M * 2 * kCb * sizeof(float), "th");
  o.in(x, (size_t)M * kCb * sizeof(float), "x");
  o.out(y, (size_t)M * kCb * sizeof(float), "y");
  TACO_TRY(o.check(who));
  return launch_highway_combine(th, x, y, M, as_stream(stream));
}
extern "C" int taco_debug_highway_combine_bwd(const float* th, const float* x, const float* dy, float* dth, float* dx, int M, void* stream) {
  const char* who = "taco_debug_highway_combine_bwd";
  DOOR_ROWS(who, "M", M);
  DoorOperands o;
  o.in(th, (size_t)M * 2 * kCb * sizeof(float), "th");
  o.in(x, (size_t)M * kCb * sizeof(float), "x");
  o.in(dy, (size_t)M * kCb * sizeof(float), "dy");
  o.out(dth, (size_t)M * 2 * kCb * sizeof(float), "dth");
  o.out(dx, (size_t)M * kCb * sizeof(float), "dx");
  TACO_TRY(o.check(who));
  return launch_highway_combine_bwd(th, x, dy, dth, dx, M, as_stream(stream));
}
// dz == dy (in place, as the model calls it) is the one overlap a door allows: dy is then checked as the output only
extern "C" int taco_debug_act_bwd(const float* y, const float* dy, const uint8_t* keep, float* dz, int64_t n, int act, void* stream) {
  const char* who = "taco_debug_act_bwd";
  TACO_REQUIRE(n > 0 && n < kDoorMaxElems, "%s: n must be in [1, 2^31), got %lld", who, (long long)n);
  TACO_REQUIRE(act >= TACO_ACT_NONE && act <= TACO_ACT_TANH, "%s: act must be one of TACO_ACT_*, got %d", who, act);
  TACO_REQUIRE(dy, "%s: dy is null", who);
  DoorOperands o;
  o.in(y, (size_t)n * sizeof(float), "y");
  if (dy != dz) o.in(dy, (size_t)n * sizeof(float), "dy");
  o.in_opt(keep, (size_t)n, "keep");
  o.out(dz, (size_t)n * sizeof(float), "dz");
  TACO_TRY(o.check(who));
  return launch_act_bwd(y, dy, keep, dz, n, act, as_stream(stream));
}
extern "C" int taco_debug_affine_act_bwd(const float* pre, const float* gamma, const float* dy, float* dz, float* dgamma, float* dbeta, int M,
                                         int N, int act, void* stream) {
  const char* who = "taco_debug_affine_act_bwd";
  DOOR_ROWS(who, "M", M);
  DOOR_COLS(who, "N", N);
  TACO_REQUIRE(act == TACO_ACT_NONE || act == TACO_ACT_RELU, "%s: act must be TACO_ACT_NONE or TACO_ACT_RELU, got %d", who, act);
  const size_t mn = (size_t)M * N * sizeof(float);
  DoorOperands o;
  o.in(pre, mn, "pre");
  o.in(gamma, (size_t)N * sizeof(float), "gamma");
  o.in(dy, mn, "dy");
  o.out(dz, mn, "dz");
  o.out(dgamma, (size_t)N * sizeof(float), "dgamma");
  o.out(dbeta, (size_t)N * sizeof(float), "dbeta");
  TACO_TRY(o.check(who));
  return launch_affine_act_bwd(pre, gamma, dy, dz, dgamma, dbeta, M, N, act, as_stream(stream));
}
extern "C" int taco_debug_mask_rows(const float* x, const int32_t* len, float* y, int B, int T, int C, void* stream) {
  const char* who = "taco_debug_mask_rows";
  TACO_REQUIRE(B > 0 && T > 0 && (int64_t)B * T <= kDoorMaxRows, "%s: B T must be in [1, 2^22], got B = %d, T = %d", who, B, T);
  DOOR_COLS4(who, "C", C);
  const size_t mc = (size_t)B * T * C * sizeof(float);
  DoorOperands o;
  o.in(x, mc, "x");
  o.in(len, (size_t)B * sizeof(int32_t), "len");
  o.out(y, mc, "y");
  TACO_TRY(o.check(who));
  return launch_mask_rows(x, len, y, B, T, C, as_stream(stream));
}
extern "C" int taco_debug_zero_tail_rows(float* x0, int C0, float* x1, int C1, const int32_t* len, int B, int Td, void* stream) {
  const char* who = "taco_debug_zero_tail_rows";
  TACO_REQUIRE(B > 0 && Td > 0 && (int64_t)B * Td <= kDoorMaxRows, "%s: B Td must be in [1, 2^22], got B = %d, Td = %d", who, B, Td);
  DOOR_COLS(who, "C0", C0);
  if (x1) DOOR_COLS(who, "C1", C1);
  DoorOperands o;
  o.out(x0, (size_t)B * Td * C0 * sizeof(float), "x0");
  o.out_opt(x1, x1 ? (size_t)B * Td * C1 * sizeof(float) : 0, "x1");
  o.in(len, (size_t)B * sizeof(int32_t), "len");
  TACO_TRY(o.check(who));
  return launch_zero_tail_rows(x0, C0, x1, C1, len, B, Td, as_stream(stream));
}
int launch_stop_rule(const float* align, const int32_t* text_length, int32_t* len, int B, int Tt, int Td, int end_offset, int hold,
                     int min_steps, hipStream_t s) {
  TACO_KLAUNCH(stop_rule_kernel, dim3(B), dim3(256), 0, s, align, text_length, len, Tt, Td, end_offset, hold, min_steps);
  TACO_LAUNCH_CHECK("stop_rule");
  return TACO_OK;
}
int launch_alignment_scores(const float* align, const int32_t* text_length, const int32_t* steps, int max_jump, int32_t* counts,
                            float* means, int B, int Td, int Tt, hipStream_t s) {
  if (Tt % 4 == 0 && (reinterpret_cast<uintptr_t>(align) & 15) == 0)
    TACO_KLAUNCH(alignment_scores_kernel<true>, dim3(B), dim3(kAlignThreads), 0, s, align, text_length, steps, max_jump, counts, means,
                 Td, Tt);
  else
    TACO_KLAUNCH(alignment_scores_kernel<false>, dim3(B), dim3(kAlignThreads), 0, s, align, text_length, steps, max_jump, counts, means,
                 Td, Tt);
  TACO_LAUNCH_CHECK("alignment_scores");
  return TACO_OK;
}
extern "C" int taco_alignment_scores(const float* alignments, const int32_t* text_length, const int32_t* steps, int max_jump,
                                     int32_t* counts, float* means, int B, int Td, int Tt, void* stream) {
  TACO_REQUIRE(alignments, "alignment_scores: alignments is NULL");
  TACO_REQUIRE(text_length, "alignment_scores: text_length is NULL");
  TACO_REQUIRE(counts, "alignment_scores: counts is NULL");
  TACO_REQUIRE(means, "alignment_scores: means is NULL");
  TACO_REQUIRE(B > 0, "alignment_scores: B=%d must be positive", B);
  TACO_REQUIRE(Td > 0, "alignment_scores: Td=%d must be positive", Td);
  TACO_REQUIRE(Tt > 0, "alignment_scores: Tt=%d must be positive", Tt);
  TACO_REQUIRE(max_jump >= 0, "alignment_scores: max_jump=%d is negative", max_jump);
  TACO_REQUIRE(Td <= TACO_ALIGNMENT_MAX_TD, "alignment_scores: Td=%d is above the %d steps one record holds", Td, TACO_ALIGNMENT_MAX_TD);
  TACO_REQUIRE(Tt <= TACO_ALIGNMENT_MAX_TT, "alignment_scores: Tt=%d is above the %d characters one bitmap holds", Tt, TACO_ALIGNMENT_MAX_TT);
  return launch_alignment_scores(alignments, text_length, steps, max_jump, counts, means, B, Td, Tt, as_stream(stream));
}
int launch_add(const float* a, const float* b, float* y, int64_t n, hipStream_t s) {
  EW_LAUNCH(add_kernel, n, s, a, b, y, n);
  return TACO_OK;
}
int launch_l1(const float* a, const float* b, float* grad, int ldg, float* loss_parts, int64_t M, int N, hipStream_t s) {
  TACO_REQUIRE(ldg >= N, "l1: ldg < N");
  // exactly kLossParts blocks: block i leaves its partial in loss_parts[i] (blocks without work write 0)
  TACO_KLAUNCH(l1_kernel, dim3(kLossParts), dim3(1024), 0, s,   // 16 waves per workgroup: the kernel is latency bound, the partial count is fixed
                     a, b, grad, ldg, loss_parts, M, N);
  TACO_LAUNCH_CHECK("l1");
  return TACO_OK;
}
int launch_finish_loss(float* loss, const float* parts, float* out, hipStream_t s) {
  TACO_KLAUNCH(finish_loss_kernel, dim3(1), dim3(kThreads), 0, s, loss, parts, out);
  TACO_LAUNCH_CHECK("finish_loss");
  return TACO_OK;
}
int launch_transpose_batch(TransposeBatch& b, hipStream_t s) {
  TACO_REQUIRE(b.n >= 1 && b.n <= kMaxTransposeBatch, "transpose_batch: %d jobs out of range", b.n);
  int tiles = 0;
  for (int i = 0; i < b.n; ++i) {
    b.j[i].tile0 = tiles;
    tiles += b.j[i].taps * ((b.j[i].N + 31) / 32) * ((b.j[i].K + 31) / 32);
  }
  TACO_KLAUNCH(transpose_batch_kernel, dim3(tiles), dim3(32, 8), 0, s, b);
  TACO_LAUNCH_CHECK("transpose_batch");
  return TACO_OK;
}
extern "C" int taco_debug_add(const float* a, const float* b, float* y, int64_t n, void* stream) {
  const char* who = "taco_debug_add";
  TACO_REQUIRE(n > 0 && n < kDoorMaxElems, "%s: n must be in [1, 2^31), got %lld", who, (long long)n);
  DoorOperands o;
  o.in(a, (size_t)n * sizeof(float), "a");
  o.in(b, (size_t)n * sizeof(float), "b");
  o.out(y, (size_t)n * sizeof(float), "y");
  TACO_TRY(o.check(who));
  return launch_add(a, b, y, n, as_stream(stream));
}
// the loss as taco_forward forms it: launch_l1 per term that is given (a term without operands contributes kLossParts zeros), then
// launch_finish_loss.  parts (2 kLossParts) and loss (3) stay with the caller.
extern "C" int taco_debug_l1_loss(const float* a0, const float* b0, float* grad0, int ldg0, int M0, int N0, const float* a1,
                                  const float* b1, float* grad1, int ldg1, int M1, int N1, float* parts, float* loss, float* out,
                                  void* stream) {
  const char* who = "taco_debug_l1_loss";
  const float* a[2] = {a0, a1};
  const float* b[2] = {b0, b1};
  float* grad[2] = {grad0, grad1};
  const int ldg[2] = {ldg0, ldg1}, M[2] = {M0, M1}, N[2] = {N0, N1};
  DoorOperands o;
  for (int i = 0; i < 2; ++i) {
    TACO_REQUIRE((a[i] != nullptr) == (b[i] != nullptr), "%s: a%d and b%d must both be given or both be null", who, i, i);
    if (!a[i]) {
      TACO_REQUIRE(!grad[i], "%s: grad%d without a%d", who, i, i);
      continue;
    }
    TACO_REQUIRE(M[i] > 0 && M[i] <= kDoorMaxRows, "%s: M%d must be in [1, 2^22], got %d", who, i, M[i]);
    TACO_REQUIRE(N[i] > 0 && N[i] <= kDoorMaxCols, "%s: N%d must be in [1, 2^14], got %d", who, i, N[i]);
    if (grad[i]) TACO_REQUIRE(ldg[i] >= N[i], "%s: ldg%d must be >= %d, got %d", who, i, N[i], ldg[i]);
    o.in(a[i], (size_t)M[i] * N[i] * sizeof(float), "a%d", i);
    o.in(b[i], (size_t)M[i] * N[i] * sizeof(float), "b%d", i);
    o.out_opt(grad[i], grad[i] ? (size_t)M[i] * ldg[i] * sizeof(float) : 0, "grad%d", i);
  }
  o.out(parts, (size_t)2 * kLossParts * sizeof(float), "parts");
  o.out(loss, 3 * sizeof(float), "loss");
  o.out_opt(out, 3 * sizeof(float), "out");
  TACO_TRY(o.check(who));
  hipStream_t s = as_stream(stream);
  for (int i = 0; i < 2; ++i) {
    if (a[i]) TACO_TRY(launch_l1(a[i], b[i], grad[i], grad[i] ? ldg[i] : N[i], parts + i * kLossParts, M[i], N[i], s));
    else TACO_TRY(taco_memset_async(parts + i * kLossParts, 0, kLossParts * sizeof(float), s, who));
  }
  return launch_finish_loss(loss, parts, out, s);
}
extern "C" int taco_debug_transpose_batch(int n, const float* const* in, float* const* out, const int* taps, const int* K, const int* N,
                                          const int* ldi, const int* ldo, void* stream) {
  const char* who = "taco_debug_transpose_batch";
  TACO_REQUIRE(n >= 1 && n <= kMaxTransposeBatch, "%s: n must be in [1, %d], got %d", who, kMaxTransposeBatch, n);
  TACO_REQUIRE(in && out && taps && K && N, "%s: a null argument table", who);
  TACO_REQUIRE((ldi != nullptr) == (ldo != nullptr), "%s: ldi and ldo must both be given or both be null", who);
  static_assert(2 * kMaxTransposeBatch <= DoorOperands::kMax, "one input and one output per job");
  TransposeBatch tb;
  DoorOperands o;
  for (int i = 0; i < n; ++i) {
    TACO_REQUIRE(taps[i] >= 1 && taps[i] <= 64, "%s: taps[%d] must be in [1, 64], got %d", who, i, taps[i]);
    TACO_REQUIRE(K[i] > 0 && K[i] <= kDoorMaxCols, "%s: K[%d] must be in [1, 2^14], got %d", who, i, K[i]);
    TACO_REQUIRE(N[i] > 0 && N[i] <= kDoorMaxCols, "%s: N[%d] must be in [1, 2^14], got %d", who, i, N[i]);
    const int li = ldi ? ldi[i] : 0, lo = ldo ? ldo[i] : 0;
    TACO_REQUIRE(li == 0 || li >= N[i], "%s: ldi[%d] must be 0 or >= %d, got %d", who, i, N[i], li);
    TACO_REQUIRE(lo == 0 || lo >= K[i], "%s: ldo[%d] must be 0 or >= %d, got %d", who, i, K[i], lo);
    TACO_REQUIRE((li == 0 && lo == 0) || taps[i] == 1, "%s: job %d has a pitch and taps = %d (a pitched job has one tap)", who, i, taps[i]);
    o.in(in[i], door_span((int64_t)taps[i] * K[i], N[i], li ? li : N[i]), "in[%d]", i);
    o.out(out[i], door_span((int64_t)taps[i] * N[i], K[i], lo ? lo : K[i]), "out[%d]", i);
    TransposeJob& J = tb.j[i];
    J.in = in[i]; J.out = out[i]; J.taps = taps[i]; J.K = K[i]; J.N = N[i]; J.tile0 = 0; J.ldi = li; J.ldo = lo;
  }
  tb.n = n;
  TACO_TRY(o.check(who));
  return launch_transpose_batch(tb, as_stream(stream));
}
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
  const uintptr_t m0 = reinterpret_cast<uintptr_t>(mag_t), o0 = reinterpret_cast<uintptr_t>(out);
  const uint64_t rows = (uint64_t)B * (uint64_t)C;   // (< 2^62; F, Fo <= 2^13: the byte counts below fit 64 bits)
  TACO_REQUIRE(rows <= (UINT64_MAX >> 16) / 4, "%s: B=%d x C=%d: the tensors exceed the address space", who, B, C);
  TACO_REQUIRE(o0 + rows * Fo * 4 <= m0 || m0 + rows * F * 4 <= o0, "%s: out overlaps mag_t", who);
  *nspan = cdiv(Fo, kStretchSpan), *ntile = cdiv(C, kStretchBins);
  *blocks = (int64_t)B * *ntile * *nspan;
  TACO_REQUIRE(*blocks <= 0x7fffffff, "%s: B=%d x C=%d x Fo=%d needs more than 2^31 workgroups", who, B, C, Fo);
  return TACO_OK;
}

// taco_frames_pitch (CURVE = false: step_q (B)) and taco_frames_pitch_curve (true: step_q (B, F)): one set of refusals, and the
// lifter path chosen by Q alone either way
template <bool CURVE>
int frames_pitch_call(const char* who, const float* mag_t, const int32_t* frames, int frames_per_unit, const int32_t* step_q, int lifter,
                      float* out, int B, int C, int F, void* stream) {
  TACO_REQUIRE(mag_t, "%s: mag_t is NULL", who);
  TACO_REQUIRE(out, "%s: out is NULL", who);
  TACO_REQUIRE(B > 0, "%s: B=%d must be positive", who, B);
  TACO_REQUIRE(C >= 9 && C <= kPitchMaxC && ((C - 1) & (C - 2)) == 0, "%s: C=%d: C - 1 must be a power of two in 8..%d", who, C,
               kPitchMaxC - 1);
  TACO_REQUIRE(F > 0 && F <= TACO_STRETCH_MAX_FRAMES, "%s: F=%d must be in 1..%d", who, F, TACO_STRETCH_MAX_FRAMES);
  const int qmax = (C - 1) / 2 < TACO_PITCH_MAX_LIFTER ? (C - 1) / 2 : TACO_PITCH_MAX_LIFTER;
  TACO_REQUIRE(lifter >= 1 && lifter <= qmax, "%s: lifter=%d must be in 1..%d at C=%d", who, lifter, qmax, C);
  TACO_REQUIRE(frames_per_unit >= 1, "%s: frames_per_unit=%d must be >= 1", who, frames_per_unit);
  const uintptr_t m0 = reinterpret_cast<uintptr_t>(mag_t), o0 = reinterpret_cast<uintptr_t>(out);
  const uint64_t bytes = (uint64_t)B * (uint64_t)C * (uint64_t)F * 4;   // (< 2^31 * 2^11 * 2^13 * 4)
  TACO_REQUIRE(o0 + bytes <= m0 || m0 + bytes <= o0, "%s: out overlaps mag_t", who);
  const int ntile = cdiv(F, kPitchFrames);
  const int64_t blocks = (int64_t)B * ntile;
  TACO_REQUIRE(blocks <= 0x7fffffff, "%s: B=%d x F=%d needs more than 2^31 workgroups", who, B, F);
  hipStream_t s = as_stream(stream);
  if (lifter <= 32)
    TACO_KLAUNCH((frames_pitch_kernel<1, 16, CURVE>), dim3((unsigned)blocks), dim3(64 * 16), 0, s, mag_t, frames, frames_per_unit, step_q,
                 lifter, out, C, F, ntile);
  else
    TACO_KLAUNCH((frames_pitch_kernel<2, 8, CURVE>), dim3((unsigned)blocks), dim3(64 * 8), 0, s, mag_t, frames, frames_per_unit, step_q,
                 lifter, out, C, F, ntile);
  TACO_LAUNCH_CHECK(who);
  return TACO_OK;
}
}  // namespace

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
  const uintptr_t m0 = reinterpret_cast<uintptr_t>(mag_t);
  const uint64_t mbytes = (uint64_t)B * (uint64_t)C * (uint64_t)F * 4, row = (uint64_t)B * (uint64_t)F * 4;
  const uintptr_t p0 = reinterpret_cast<uintptr_t>(period), s0 = reinterpret_cast<uintptr_t>(strength),
                  a0 = reinterpret_cast<uintptr_t>(acf);
  TACO_REQUIRE(p0 + row <= m0 || m0 + mbytes <= p0, "frames_f0: period overlaps mag_t");
  TACO_REQUIRE(s0 + row <= m0 || m0 + mbytes <= s0, "frames_f0: strength overlaps mag_t");
  TACO_REQUIRE(!acf || a0 + row * (uint64_t)L <= m0 || m0 + mbytes <= a0, "frames_f0: acf overlaps mag_t");
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
// The widest access taco_corpus_batch may use: the largest V in {8 (fp16 only), 4, 2, 1} that divides the row pitch, with the
// source base a multiple of V elements and the output base a multiple of min(V, 4) floats (lib.corpus_batch_width restates it).
static int corpus_batch_width(const void* src, int src_fp16, const float* out, int64_t row) {
  const uintptr_t sa = reinterpret_cast<uintptr_t>(src), oa = reinterpret_cast<uintptr_t>(out);
  const int esz = src_fp16 ? 2 : 4;
  for (int v = src_fp16 ? 8 : 4; v > 1; v >>= 1)
    if (row % v == 0 && sa % (uintptr_t)(v * esz) == 0 && oa % (uintptr_t)((v < 4 ? v : 4) * 4) == 0) return v;
  return 1;
}
template <typename T, int V>
static void corpus_batch_launch(const void* src, const int64_t* index, const float* mean, const float* stdv, float* out,
                                int32_t* n_bad, int64_t N, int B, int64_t row, int C, int chunks, hipStream_t s) {
  const int step = (256 * V) % C;
  const dim3 grid((unsigned)((int64_t)B * chunks));
  if (mean)
    TACO_KLAUNCH((corpus_batch_kernel<T, V, true>), grid, dim3(256), 0, s, static_cast<const T*>(src), index, mean, stdv, out,
                 n_bad, N, row, C, step, chunks);
  else
    TACO_KLAUNCH((corpus_batch_kernel<T, V, false>), grid, dim3(256), 0, s, static_cast<const T*>(src), index, mean, stdv, out,
                 n_bad, N, row, C, step, chunks);
}
extern "C" int taco_corpus_batch(const void* src, int src_fp16, const int64_t* index, const float* mean, const float* stdv,
                                 float* out, int32_t* n_bad, int64_t N, int B, int64_t row, int C, void* stream) {
  TACO_REQUIRE(src, "corpus_batch: src is NULL");
  TACO_REQUIRE(out, "corpus_batch: out is NULL");
  TACO_REQUIRE(N > 0, "corpus_batch: N=%lld must be positive", (long long)N);
  TACO_REQUIRE(B > 0, "corpus_batch: B=%d must be positive", B);
  TACO_REQUIRE(row > 0, "corpus_batch: row=%lld must be positive", (long long)row);
  TACO_REQUIRE(C > 0, "corpus_batch: C=%d must be positive", C);
  TACO_REQUIRE(row % C == 0, "corpus_batch: row=%lld is not a multiple of C=%d", (long long)row, C);
  TACO_REQUIRE((mean == nullptr) == (stdv == nullptr), "corpus_batch: mean and std must both be given or both be NULL");
  TACO_REQUIRE(index || B <= N, "corpus_batch: index is NULL (identity) but B=%d exceeds N=%lld", B, (long long)N);
  const int esz = src_fp16 ? 2 : 4;
  const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), o0 = reinterpret_cast<uintptr_t>(out);
  TACO_REQUIRE(N <= INT64_MAX / row / esz && (int64_t)B <= INT64_MAX / row / 4, "corpus_batch: N, B, row: the tensors exceed the address space");
  TACO_REQUIRE(o0 + (uintptr_t)B * row * 4 <= s0 || s0 + (uintptr_t)N * row * esz <= o0, "corpus_batch: out overlaps src");
  const int V = corpus_batch_width(src, src_fp16, out, row);
  const int64_t per = (int64_t)kCorpusU * 256 * V;
  const int64_t chunks = (row + per - 1) / per;
  TACO_REQUIRE((int64_t)B * chunks <= 0x7fffffff, "corpus_batch: B=%d x row=%lld needs more than 2^31 workgroups", B, (long long)row);
  hipStream_t s = as_stream(stream);
  if (n_bad) TACO_TRY(taco_memset_async(n_bad, 0, sizeof(int32_t), s, "corpus_batch"));
#define CORPUS_BATCH_CASE(T, v) \
  case v: corpus_batch_launch<T, v>(src, index, mean, stdv, out, n_bad, N, B, row, C, (int)chunks, s); break
  if (src_fp16) {
    switch (V) {
      CORPUS_BATCH_CASE(_Float16, 8);
      CORPUS_BATCH_CASE(_Float16, 4);
      CORPUS_BATCH_CASE(_Float16, 2);
      CORPUS_BATCH_CASE(_Float16, 1);
    }
  } else {
    switch (V) {
      CORPUS_BATCH_CASE(float, 4);
      CORPUS_BATCH_CASE(float, 2);
      CORPUS_BATCH_CASE(float, 1);
    }
  }
#undef CORPUS_BATCH_CASE
  TACO_LAUNCH_CHECK("corpus_batch");
  return TACO_OK;
}
int launch_sumsq(const float* x, int64_t n, float* out, hipStream_t s) {
  TACO_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0, "sumsq: x must be 16-byte aligned");
  // one block per CU, one partial each
  TACO_KLAUNCH(sumsq_kernel, dim3(kSumsqParts), dim3(kThreads), 0, s, x, n, out);
  TACO_LAUNCH_CHECK("sumsq");
  return TACO_OK;
}
extern "C" int taco_debug_sumsq(const float* x, int64_t n, float* out, void* stream) {
  const char* who = "taco_debug_sumsq";
  TACO_REQUIRE(n > 0 && n < kDoorMaxElems, "%s: n must be in [1, 2^31), got %lld", who, (long long)n);
  DoorOperands o;
  o.in(x, (size_t)n * sizeof(float), "x");
  o.out(out, (size_t)kSumsqParts * sizeof(float), "out");
  TACO_TRY(o.check(who));
  return launch_sumsq(x, n, out, as_stream(stream));
}
int launch_clip_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float cap, int64_t step,
                     const float* sumsq, float* gnorm_out, const int32_t* err, hipStream_t s) {
  const double b1 = 0.9, b2 = 0.999;
  const double lr_t = (double)lr * sqrt(1.0 - pow(b2, (double)step)) / (1.0 - pow(b1, (double)step));
  TACO_KLAUNCH(clip_adam_kernel, dim3(grid_for(n, kThreads, 2048)), dim3(kThreads), 0, s, p, g, m, v, n,
                     (float)lr_t, cap, sumsq, gnorm_out, err);
  TACO_LAUNCH_CHECK("clip_adam");
  return TACO_OK;
}
extern "C" int taco_fill_bernoulli(uint8_t* out, int64_t n, float p_one, uint64_t seed, void* stream) {
  TACO_REQUIRE(out && n > 0, "fill_bernoulli: bad arguments");
  hipStream_t s = as_stream(stream);
  double t = (double)p_one * 4294967296.0;
  uint32_t thresh = t >= 4294967295.0 ? 0xFFFFFFFFu : (t <= 0 ? 0u : (uint32_t)t);
  TACO_KLAUNCH(bernoulli_kernel, dim3(grid_for((n + 1) / 2)), dim3(kThreads), 0, s, out, n, thresh, seed);
  TACO_LAUNCH_CHECK("bernoulli");
  return TACO_OK;
}

// ---- communication-kernel stand-in (taco_debug_spin): `blocks` workgroups of `threads` threads holding `lds_bytes` of LDS
//      each, spinning for `usec` microseconds of wall time.  The footprint of a collective kernel for co-residency tests of
//      the persistent decoder launches (tests/test_gpu_dist.py); does no work.
__global__ void spin_kernel(long long ticks, int lds_words) {
  extern __shared__ __attribute__((aligned(16))) int spin_lds[];
  for (int i = threadIdx.x; i < lds_words; i += blockDim.x) spin_lds[i] = i;   // touch the allocation
  __syncthreads();
  const long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(16);
  if (lds_words > 0 && spin_lds[(threadIdx.x * 7) % lds_words] == -12345) spin_lds[0] = 1;   // keeps the touch alive
}
extern "C" int taco_debug_spin(int blocks, int threads, int lds_bytes, int usec, void* stream) {
  TACO_REQUIRE(blocks > 0 && threads > 0 && threads <= 1024 && lds_bytes >= 0 && lds_bytes <= 160 * 1024 && usec >= 0,
               "debug_spin: bad arguments");
  hipStream_t s = as_stream(stream);
  if (lds_bytes > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(spin_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    if (e != hipSuccess) {
      taco_set_error("debug_spin: hipFuncSetAttribute: %s", hipGetErrorString(e));
      return TACO_ELAUNCH;
    }
  }
  int rate_khz = 100000;   // wall_clock64 ticks at the constant s_memrealtime rate (100 MHz on gfx950); ask the runtime
  int dev = 0;
  if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&rate_khz, hipDeviceAttributeWallClockRate, dev);
  if (rate_khz <= 0) rate_khz = 100000;
  TACO_KLAUNCH(spin_kernel, dim3(blocks), dim3(threads), (size_t)lds_bytes, s, (long long)usec * rate_khz / 1000, lds_bytes / 4);
  TACO_LAUNCH_CHECK("debug_spin");
  return TACO_OK;
}

// ---- shader-clock probe (taco_debug_clock_probe): every CU runs one 512-thread workgroup whose waves each walk a chain of
//      `iters` dependent v_fma_f32 -- the occupancy and issue pattern of the persistent decoder kernels, without their memory
//      traffic -- and workgroup 0 reports the elapsed shader cycles (s_memtime) and constant-rate ticks (s_memrealtime, 100 MHz).
//      cycles / time = the clock this chip sustains under a chip-wide LATENCY-BOUND load, which is what the decoder and bi-GRU
//      kernels scale with; boxes of one pool differ (round 4: the same build ran 8.86 and 9.30 ms per step).
__global__ __launch_bounds__(512) void clock_probe_kernel(long long* out, int iters, float a, float b) {
  float x = (float)threadIdx.x;
  const long long c0 = clock64(), w0 = wall_clock64();
  for (int i = 0; i < iters; i += 16) {
#pragma unroll
    for (int j = 0; j < 16; ++j) x = fmaf(x, a, b);
  }
  const long long c1 = clock64(), w1 = wall_clock64();
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    out[0] = c1 - c0;
    out[1] = w1 - w0;
  }
  if (x == 12345.678f) out[2] = 1;   // keeps the chain alive
}
extern "C" int taco_debug_clock_probe(long long* out, int iters, void* stream) {   // out[0] = shader cycles, out[1] = 100 MHz ticks
  TACO_REQUIRE(out && iters > 0, "clock_probe: bad arguments");
  hipStream_t s = as_stream(stream);
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  TACO_KLAUNCH(clock_probe_kernel, dim3(cus > 0 ? cus : 256), dim3(512), 0, s, out, iters, 0.999f, 0.001f);
  TACO_LAUNCH_CHECK("clock_probe");
  return TACO_OK;
}

// ---- fabric probe (taco_debug_fabric_probe): what the latency-bound kernels of this library actually wait on, measured on THIS
//      box (the shader clock does not tell a 12.4 us BPTT box from a 14.0 us one).  One launch, 64 workgroups of 64
//      threads (workgroup b runs on XCD b % 8 with the dispatcher's round-robin; the XCC ids are recorded, not assumed):
//        blocks 0 <-> 8   ping-pong through an 8-byte {epoch, value} granule in decoder3's fast form: workgroup-scope store
//                         (stays in the XCD's L2) + agent-scope load (bypasses L1)                     -> out[0] ticks / hop pair
//        blocks 1 <-> 9   the same with agent-scope stores (written through; decoder3's fallback form) -> out[1]
//        blocks 2 <-> 3   agent scope, two DIFFERENT XCDs (decoder.hip's exchange)                     -> out[2]
//        block  20        a chain of dependent loads over a warm 64 KB region (L2 hits)                 -> out[3]
//        block  21        a chain of dependent AGENT-SCOPE loads over the whole scratch buffer (cold lines: the memory-side
//                         round trip an L2-bypassing load pays when no peer has just written the line)          -> out[4]
//        block  22        64 lanes streaming 8 MB of the scratch buffer with 16-byte loads (one CU's stream bandwidth) -> out[5]
//      Ticks are the constant 100 MHz counter; out[8 + b] = XCC id of block b (b < 24); out[6] = iterations, out[7] = ok flags.
typedef unsigned long long fp_u64;
typedef __attribute__((address_space(1))) fp_u64 fp_gu64;
template <int LSCOPE, int SSCOPE>
__device__ __forceinline__ long long fabric_pingpong(fp_u64* mine, fp_u64* theirs, bool first, int iters, bool* ok_out) {
  bool ok = true;
  const long long t0 = wall_clock64();
  for (int i = 1; i <= iters && ok; ++i) {
    if (first) __hip_atomic_store((fp_gu64*)mine, ((fp_u64)i << 32) | (fp_u64)i, __ATOMIC_RELAXED, SSCOPE);
    ok = false;
    for (unsigned spin = 0; spin < (1u << 20); ++spin) {
      const fp_u64 x = __hip_atomic_load((fp_gu64*)theirs, __ATOMIC_RELAXED, LSCOPE);
      if ((unsigned)(x >> 32) == (unsigned)i) { ok = true; break; }
    }
    if (!first) __hip_atomic_store((fp_gu64*)mine, ((fp_u64)i << 32) | (fp_u64)i, __ATOMIC_RELAXED, SSCOPE);
  }
  *ok_out = ok;
  return wall_clock64() - t0;
}
__global__ __launch_bounds__(64) void fabric_probe_kernel(long long* out, fp_u64* gran, const unsigned* scratch, long long scratch_words, int iters) {
  const int b = blockIdx.x;
  if (threadIdx.x == 0 && b < 24) {
    unsigned id;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(id));
    out[8 + b] = id & 0xf;
  }
  if (b == 22) {   // one CU streaming: 8 MB, 16 bytes per lane and load, 8 loads in flight per lane
    typedef unsigned fp_u32x4 __attribute__((ext_vector_type(4)));
    const fp_u32x4* src = reinterpret_cast<const fp_u32x4*>(scratch);
    const long long n16 = (8ll << 20) / 16;
    unsigned acc = 0;
    const long long t0 = wall_clock64();
    for (long long i = threadIdx.x; i + 7 * 64 < n16; i += 8 * 64) {
      fp_u32x4 v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = __builtin_nontemporal_load(src + i + j * 64);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc += v[j][0] ^ v[j][3];
    }
    const long long t1 = wall_clock64();
    if (threadIdx.x == 0) out[5] = t1 - t0;
    if (acc == 0x12345678u) out[7] |= 1ll << 40;
    return;
  }
  if (threadIdx.x != 0) return;
  bool ok = true;
  if (b == 0 || b == 8) {
    const long long t = fabric_pingpong<__HIP_MEMORY_SCOPE_AGENT, __HIP_MEMORY_SCOPE_WORKGROUP>(gran + (b == 0 ? 0 : 64), gran + (b == 0 ? 64 : 0), b == 0, iters, &ok);
    if (b == 0) { out[0] = t; if (ok) atomicOr((unsigned long long*)&out[7], 1ull); }
  } else if (b == 1 || b == 9) {
    const long long t = fabric_pingpong<__HIP_MEMORY_SCOPE_AGENT, __HIP_MEMORY_SCOPE_AGENT>(gran + (b == 1 ? 128 : 192), gran + (b == 1 ? 192 : 128), b == 1, iters, &ok);
    if (b == 1) { out[1] = t; if (ok) atomicOr((unsigned long long*)&out[7], 2ull); }
  } else if (b == 2 || b == 3) {
    const long long t = fabric_pingpong<__HIP_MEMORY_SCOPE_AGENT, __HIP_MEMORY_SCOPE_AGENT>(gran + (b == 2 ? 256 : 320), gran + (b == 2 ? 320 : 256), b == 2, iters, &ok);
    if (b == 2) { out[2] = t; if (ok) atomicOr((unsigned long long*)&out[7], 4ull); }
  } else if (b == 20 || b == 21) {
    // dependent loads: the next index is a multiplicative walk over the region PLUS the loaded word (the buffer holds zeros, which
    // the compiler cannot know), 32 words = one 128-byte line apart.  The L2-hit walk covers 64 KB and touches every line once
    // before the clock starts (64 KB exceeds the CU's L1: the walk is served by the XCD's L2); plain loads -- agent-scope loads
    // were measured to take the same ~320 ns whether the line is in the L2 or nowhere, i.e. they are fabric round trips
    long long lines = (b == 20 ? (64ll << 10) : scratch_words * 4) / 128;
    while (lines & (lines - 1)) lines &= lines - 1;   // largest power of two: the walk is a mask, not a 64-bit software modulo
    const unsigned long long mask = (unsigned long long)lines - 1;
    unsigned long long idx = 1;
    if (b == 20) {
      unsigned w = 0;
      for (long long l = 0; l < lines; ++l)
        w += scratch[(16ll << 20) / 4 + l * 32];
      idx += w;
    }
    const unsigned* base = b == 20 ? scratch + (16ll << 20) / 4 : scratch;   // (the streaming block reads the first 8 MB)
    const long long t0 = wall_clock64();
    for (int i = 0; i < iters; ++i) {
      // block 20: a plain load (served by the L2 after the warm-up); block 21: an agent-scope load, which bypasses L1 AND is
      // not served from another XCD's L2 -- the kind of load every exchange poll is, here on lines nobody has written lately
      const unsigned v = b == 20 ? base[idx * 32]
                                 : __hip_atomic_load((const __attribute__((address_space(1))) unsigned*)(base + idx * 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      idx = (idx * 1664525ull + 1013904223ull + v) & mask;   // (full-period LCG modulo 2^k)
    }
    const long long t1 = wall_clock64();
    out[b == 20 ? 3 : 4] = t1 - t0;
    if (idx == 0xfffffffffull) out[7] |= 1ll << 41;
  }
  if (b == 0) out[6] = iters;
}
extern "C" int taco_debug_fabric_probe(long long* out32, void* gran4k, const void* scratch, long long scratch_bytes, int iters,
                                       void* stream) {
  TACO_REQUIRE(out32 && gran4k && scratch && scratch_bytes >= (32 << 20) && iters > 0, "fabric_probe: bad arguments");
  hipStream_t s = as_stream(stream);
  TACO_KLAUNCH(fabric_probe_kernel, dim3(64), dim3(64), 0, s, out32, reinterpret_cast<fp_u64*>(gran4k),
                     reinterpret_cast<const unsigned*>(scratch), (long long)(scratch_bytes / 4), iters);
  TACO_LAUNCH_CHECK("fabric_probe");
  return TACO_OK;
}

// ---- batched zero-fill / copy (InitBatch, kernels.h) ----
__global__ __launch_bounds__(256) void init_batch_kernel(InitBatch b) {
  int ji = 0;
#pragma unroll 1
  for (int i = 1; i < b.n; ++i)
    if ((int)blockIdx.x >= b.j[i].blk0) ji = i;
  const InitJob& q = b.j[ji];
  const int nb = (ji + 1 < b.n ? b.j[ji + 1].blk0 : (int)gridDim.x) - q.blk0;
  const int64_t total = (int64_t)q.rows * q.cols;
  const bool vec = (q.cols % 4 == 0) && (q.ldd % 4 == 0) && (q.lds % 4 == 0) && ((reinterpret_cast<uintptr_t>(q.dst) & 15) == 0) &&
                   (q.src == nullptr || (reinterpret_cast<uintptr_t>(q.src) & 15) == 0);
  if (vec) {
    const int64_t c4 = q.cols / 4, n4 = total / 4;
    for (int64_t i = (int64_t)(blockIdx.x - q.blk0) * 256 + threadIdx.x; i < n4; i += (int64_t)nb * 256) {
      const int64_t r = i / c4, c = (i - r * c4) * 4;
      const float4 v = q.src ? *reinterpret_cast<const float4*>(q.src + r * q.lds + c) : make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(q.dst + r * q.ldd + c) = v;
    }
  } else {
    for (int64_t i = (int64_t)(blockIdx.x - q.blk0) * 256 + threadIdx.x; i < total; i += (int64_t)nb * 256) {
      const int64_t r = i / q.cols, c = i - r * q.cols;
      q.dst[r * q.ldd + c] = q.src ? q.src[r * q.lds + c] : 0.f;
    }
  }
}
int launch_init_batch(InitBatch& b, hipStream_t s) {
  if (b.n == 0) return TACO_OK;
  int blocks = 0;
  for (int i = 0; i < b.n; ++i) {
    b.j[i].blk0 = blocks;
    const int64_t total = (int64_t)b.j[i].rows * b.j[i].cols;
    int64_t nb = (total + 256 * 16 - 1) / (256 * 16);      // 16 floats (4 float4) per thread at most
    nb = nb < 1 ? 1 : (nb > 2048 ? 2048 : nb);
    blocks += (int)nb;
  }
  TACO_KLAUNCH(init_batch_kernel, dim3(blocks), dim3(256), 0, s, b);
  TACO_LAUNCH_CHECK("init_batch");
  b.n = 0;
  return TACO_OK;
}
