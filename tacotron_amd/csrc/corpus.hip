// corpus.hip -- the corpus feed (include/taco_hip.h taco_corpus_batch): a training batch gathered from the corpus as it is stored in
// HBM (fp16 or fp32 rows) and standardised in the same pass.
#include "common.h"
#include "kernels.h"

namespace {

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

}  // namespace

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
  TACO_REQUIRE(N <= INT64_MAX / row / esz && (int64_t)B <= INT64_MAX / row / 4, "corpus_batch: N, B, row: the tensors exceed the address space");
  TACO_REQUIRE(!bytes_meet(out, (uint64_t)B * row * 4, src, (uint64_t)N * row * esz), "corpus_batch: out overlaps src");
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
