// elementwise.hip -- HBM-bound glue kernels of the train step: embedding gather/scatter (tacotron.py:111-114),
// BN-affine + max-pool (ops.py:64-71), highway blend (ops.py:46), activation/dropout derivatives, column reductions
// for bias / BN gradients, row masks, L1 loss + sign gradient (tacotron.py:158-160), weight transposes for the backward GEMMs,
// global-norm clip + TF-form Adam (tacotron.py:167-185), the Bernoulli mask generator and the batched zero-fill / copy, with their
// launchers and op-level debug doors.
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
