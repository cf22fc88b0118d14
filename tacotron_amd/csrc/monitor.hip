// monitor.hip -- per-tensor statistics and sign-symmetric log histograms of many segments of one fp32 buffer in one call
// (include/taco_hip.h taco_tensor_stats and its plan / size functions).  The reference attaches tf.summary.histogram to eight
// activations (models/tacotron.py:129,139,152, models/ops.py:73-130); here the same pass also serves the parameters, the gradients and
// both Adam slots, whose flat buffers taco_param_table describes.
//
// A segment (offset, size) is laid on POSITIONS p = (offset & 3) + j, j its element index: position 0 is the 16-byte boundary at or
// below its first float (base itself is 16-byte aligned).  Chunk c of the segment is the positions [c C, (c + 1) C), C =
// TACO_STATS_CHUNK, so the cut depends on the segment's own descriptor alone.  A work item is one (segment, chunk) and belongs to one
// WAVE; a workgroup of four waves takes four consecutive items of the host-built plan, whatever segments they belong to -- a bias of
// 128 floats costs a wave, not a workgroup.
//   stats_items_kernel  lane l of the wave owns the groups of four positions g = l, l + 64, ... of the chunk (32 of them): a whole
//                       group is one 16-byte load, the two edge groups of a segment scalar loads.  Per lane: the counters, the fp64
//                       sum and sum of squares in increasing position, the extremes as ordered integer keys; per wave: a private
//                       histogram in LDS (integer adds).  Lanes meet in a fixed tree.  -> one record per item; the waves of a
//                       workgroup that hold consecutive chunks of one segment add their histograms and write ONE row
//   stats_fold_kernel   per segment: the records 64 chunks at a time in chunk order (lane l the chunk c0 + l, the same tree, then the
//                       running total) in a workgroup of its own, the histogram rows summed as integers (exact in any order), 64
//                       bins per workgroup -> counts, moments, hist
// No float atomics and no global atomics at all; every word of the workspace that the fold reads was written by the first launch.
#include <math.h>
#include <string.h>

#include "kernels.h"

namespace {

constexpr int MS_C = TACO_STATS_CHUNK;       // positions per work item
constexpr int MS_WAVES = 4;                  // items per workgroup
constexpr int MS_T = 64 * MS_WAVES;
constexpr int MS_GROUPS = MS_C / 4 / 64;     // 16-byte groups per lane
constexpr int MS_FT = 512;                   // fold block
constexpr int MS_BATCH = 8;                  // 16-byte loads a lane has in flight inside a whole chunk
constexpr int MS_BINS = 64;                  // histogram bins per fold workgroup
constexpr int64_t MS_MAGIC = 0x31534e4154534f43ll;
constexpr int64_t MS_MAX_SIZE = (int64_t)1 << 40;
static_assert(MS_C % 256 == 0 && MS_GROUPS % MS_BATCH == 0, "a chunk is whole rounds of 64 lanes x 4 floats, in whole batches");

struct MsHeader { int64_t magic, n, n_items, base_floats; };
struct MsSeg { int64_t offset, size, item0, chunks; };
struct MsItem { int32_t seg, chunk; };
// what a wave leaves of its chunk (the centre bin's count travels in the histogram row)
struct MsRec {
  uint32_t finite, nan, pinf, ninf, zeros, kmin, kmax, umax;
  double sum, sumsq;
};
static_assert(sizeof(MsRec) == 48, "record layout");

struct MsBuckets { uint32_t lo, hi; int shift, nm, nb; };

// finite floats as unsigned keys in their order, -0 below +0
__device__ __forceinline__ uint32_t ms_key(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }
__device__ __forceinline__ float ms_unkey(uint32_t key) { return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key); }

struct MsAcc {
  uint32_t finite = 0, nan = 0, pinf = 0, ninf = 0, zeros = 0, mid = 0;
  uint32_t kmin = 0xffffffffu, kmax = 0u, umax = 0u;
  double sum = 0.0, sumsq = 0.0;
};

__device__ __forceinline__ void ms_take(MsAcc& a, float x, bool valid, const MsBuckets& q, uint32_t* __restrict__ h) {
  const uint32_t bits = __float_as_uint(x), u = bits & 0x7fffffffu;
  const bool fin = valid && u < 0x7f800000u;
  a.finite += fin;
  a.nan += valid && u > 0x7f800000u;
  a.pinf += valid && bits == 0x7f800000u;
  a.ninf += valid && bits == 0xff800000u;
  a.zeros += valid && u == 0u;
  const double xd = fin ? (double)x : 0.0;   // (x + 0.0 is x: the running sums are never -0)
  a.sum += xd;
  a.sumsq = fma(xd, xd, a.sumsq);            // the square of an fp32 value is exact in fp64: one rounding, that of the sum
  if (fin) {
    const uint32_t key = ms_key(bits);
    a.kmin = min(a.kmin, key);
    a.kmax = max(a.kmax, key);
    a.umax = max(a.umax, u);
    const uint32_t k = u >> q.shift;
    if (k < q.lo) {
      ++a.mid;
    } else {
      const int m = (int)(min(k, q.hi) - q.lo) + 1;
      atomicAdd(&h[q.nm + ((bits >> 31) ? -m : m)], 1u);   // LDS, integer: exact
    }
  }
}

__device__ __forceinline__ uint32_t ms_wave_add(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;
}
__device__ __forceinline__ uint32_t ms_wave_min(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_down(v, o));
  return v;
}
__device__ __forceinline__ uint32_t ms_wave_max(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_down(v, o));
  return v;
}
// THE tree of the header: v_l += v_(l + 32), then + 16, 8, 4, 2, 1; lane 0 holds the total
__device__ __forceinline__ double ms_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_down(v, o);
  return v;
}

__global__ __launch_bounds__(MS_T) void stats_items_kernel(const float* __restrict__ base, const MsSeg* __restrict__ segs,
                                                           const MsItem* __restrict__ items, int n_items, const MsBuckets q,
                                                           MsRec* __restrict__ recs, uint32_t* __restrict__ part) {
  extern __shared__ uint32_t ms_lds[];   // MS_WAVES x nb
  __shared__ uint32_t sh_mid[MS_WAVES];
  __shared__ int sh_cont[MS_WAVES];      // the wave's item continues the segment of the wave in front of it
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int item = blockIdx.x * MS_WAVES + w;
  const bool has = item < n_items;       // (uniform in the wave; every wave reaches both barriers)
  uint32_t* h = ms_lds + (size_t)w * q.nb;
  for (int b = lane; b < q.nb; b += 64) h[b] = 0u;
  __syncthreads();
  MsAcc a;
  bool cont = false;
  if (has) {
    const MsItem it = items[item];
    const MsSeg sg = segs[it.seg];
    const int64_t lo = sg.offset & 3, hi = lo + sg.size;   // the segment's positions
    const float* p0 = base + (sg.offset - lo);             // position 0: 16-byte aligned
    const int64_t P = (int64_t)it.chunk * MS_C;
    cont = it.chunk > 0;
    if (P >= lo && P + MS_C <= hi) {   // (uniform) a chunk inside the segment: MS_BATCH loads in flight, then their floats in order
      const float4* src = reinterpret_cast<const float4*>(p0 + P) + lane;
      for (int r0 = 0; r0 < MS_GROUPS; r0 += MS_BATCH) {
        float4 v[MS_BATCH];
#pragma unroll
        for (int k = 0; k < MS_BATCH; ++k) v[k] = src[(r0 + k) * 64];
#pragma unroll
        for (int k = 0; k < MS_BATCH; ++k) {
          ms_take(a, v[k].x, true, q, h);
          ms_take(a, v[k].y, true, q, h);
          ms_take(a, v[k].z, true, q, h);
          ms_take(a, v[k].w, true, q, h);
        }
      }
    } else {   // a segment's first or last chunk: the same floats in the same order, group by group
#pragma unroll 4
      for (int r = 0; r < MS_GROUPS; ++r) {
        const int64_t pos = P + (int64_t)(r * 64 + lane) * 4;
        if (pos >= lo && pos + 4 <= hi) {
          const float4 v = *reinterpret_cast<const float4*>(p0 + pos);
          ms_take(a, v.x, true, q, h);
          ms_take(a, v.y, true, q, h);
          ms_take(a, v.z, true, q, h);
          ms_take(a, v.w, true, q, h);
        } else if (pos + 4 > lo && pos < hi) {   // an edge group: only the floats of the segment are read
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const bool valid = pos + k >= lo && pos + k < hi;
            const float x = valid ? p0[pos + k] : 0.f;
            ms_take(a, x, valid, q, h);
          }
        }
      }
    }
  }
  const uint32_t mid = __shfl(ms_wave_add(a.mid), 0);   // the centre bin: nobody adds to it in LDS
  MsRec rec;
  rec.finite = ms_wave_add(a.finite);
  rec.nan = ms_wave_add(a.nan);
  rec.pinf = ms_wave_add(a.pinf);
  rec.ninf = ms_wave_add(a.ninf);
  rec.zeros = ms_wave_add(a.zeros);
  rec.kmin = ms_wave_min(a.kmin);
  rec.kmax = ms_wave_max(a.kmax);
  rec.umax = ms_wave_max(a.umax);
  rec.sum = ms_wave_sum(a.sum);
  rec.sumsq = ms_wave_sum(a.sumsq);
  if (lane == 0) {
    sh_mid[w] = mid;
    sh_cont[w] = cont;
  }
  __syncthreads();   // every wave's LDS adds are done
  if (!has) return;
  if (lane == 0) recs[item] = rec;
  // one histogram row per run of waves that hold consecutive chunks of one segment, written as the row of the run's first item
  // (integer adds: exact in any order).  The fold reads the rows of exactly these items: chunk 0, and the first wave of a workgroup
  if (w > 0 && cont) return;
  int run = 1;
  while (w + run < MS_WAVES && sh_cont[w + run]) ++run;
  uint32_t* row = part + (int64_t)item * q.nb;
  for (int b = lane; b < q.nb; b += 64) {
    uint32_t v = 0u;
    for (int k = 0; k < run; ++k) v += b == q.nm ? sh_mid[w + k] : h[(size_t)k * q.nb + b];
    row[b] = v;
  }
}

// grid (n, ceil(nb / 64) + 1): the histogram bins [64 y, 64 y + 64) of segment x; the last y its counts and moments
__global__ __launch_bounds__(MS_FT) void stats_fold_kernel(const MsSeg* __restrict__ segs, int nb, const MsRec* __restrict__ recs,
                                                           const uint32_t* __restrict__ part, int64_t* __restrict__ counts,
                                                           double* __restrict__ moments, int64_t* __restrict__ hist, int tiles) {
  __shared__ unsigned long long sh[MS_FT / 64][MS_BINS];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int s = blockIdx.x;
  const MsSeg sg = segs[s];
  if ((int)blockIdx.y < tiles) {
    const int bin = blockIdx.y * MS_BINS + lane;
    unsigned long long acc = 0;
    if (bin < nb && sg.chunks > 0) {
      // the rows that exist: chunk 0's, and those of the items that are the first of their workgroup (stats_items_kernel)
      const uint32_t* col = part + sg.item0 * nb + bin;
      if (w == 0) acc = col[0];
      int64_t first = (MS_WAVES - sg.item0 % MS_WAVES) % MS_WAVES;
      if (first == 0) first = MS_WAVES;
#pragma unroll 4
      for (int64_t c = first + (int64_t)MS_WAVES * w; c < sg.chunks; c += (int64_t)MS_WAVES * (MS_FT / 64)) acc += col[c * nb];
    }
    sh[w][lane] = acc;
    __syncthreads();
    if (w != 0 || bin >= nb) return;
    for (int k = 1; k < MS_FT / 64; ++k) acc += sh[k][lane];
    hist[(int64_t)s * nb + bin] = (int64_t)acc;
    return;
  }
  if (w != 0) return;
  unsigned long long finite = 0, nan = 0, pinf = 0, ninf = 0, zeros = 0;
  uint32_t kmin = 0xffffffffu, kmax = 0u, umax = 0u;
  double sum = 0.0, sumsq = 0.0;
  const MsRec none = {0u, 0u, 0u, 0u, 0u, 0xffffffffu, 0u, 0u, 0.0, 0.0};
  MsRec next = lane < sg.chunks ? recs[sg.item0 + lane] : none;
  for (int64_t c0 = 0; c0 < sg.chunks; c0 += 64) {   // (uniform)
    const MsRec r = next;
    next = c0 + 64 + lane < sg.chunks ? recs[sg.item0 + c0 + 64 + lane] : none;   // (in flight while this tile is reduced)
    finite += ms_wave_add(r.finite);   // (a chunk holds at most C elements: 64 of them fit 32 bits)
    nan += ms_wave_add(r.nan);
    pinf += ms_wave_add(r.pinf);
    ninf += ms_wave_add(r.ninf);
    zeros += ms_wave_add(r.zeros);
    kmin = min(kmin, ms_wave_min(r.kmin));
    kmax = max(kmax, ms_wave_max(r.kmax));
    umax = max(umax, ms_wave_max(r.umax));
    sum = sum + ms_wave_sum(r.sum);
    sumsq = sumsq + ms_wave_sum(r.sumsq);
  }
  if (lane != 0) return;
  int64_t* cn = counts + 6 * (int64_t)s;
  cn[0] = sg.size;
  cn[1] = (int64_t)finite;
  cn[2] = (int64_t)nan;
  cn[3] = (int64_t)pinf;
  cn[4] = (int64_t)ninf;
  cn[5] = (int64_t)zeros;
  double* mo = moments + 5 * (int64_t)s;
  mo[0] = sum;
  mo[1] = sumsq;
  mo[2] = finite ? (double)ms_unkey(kmin) : (double)INFINITY;
  mo[3] = finite ? (double)ms_unkey(kmax) : -(double)INFINITY;
  mo[4] = finite ? (double)__uint_as_float(umax) : 0.0;
}

// ---- host: the plan ------------------------------------------------------------------------------------------------------------
int64_t ms_chunks(int64_t offset, int64_t size) { return size > 0 ? ((offset & 3) + size + MS_C - 1) / MS_C : 0; }

// the items of n segments, or -1 for a descriptor no plan takes (base_floats < 0: the range check is left to the caller)
int64_t ms_count_items(const int64_t* segments, int n, int64_t base_floats) {
  int64_t items = 0;
  for (int i = 0; i < n; ++i) {
    const int64_t off = segments[2 * i], size = segments[2 * i + 1];
    if (off < 0 || size < 0 || size > MS_MAX_SIZE || off > MS_MAX_SIZE) return -1;
    if (base_floats >= 0 && off + size > base_floats) return -1;
    items += ms_chunks(off, size);
  }
  return items;
}

bool ms_buckets(int e_lo, int e_hi, int sub_bits, MsBuckets& q) {
  if (sub_bits < 0 || sub_bits > 3 || e_lo < -126 || e_hi > 127 || e_lo > e_hi) return false;
  q.shift = 23 - sub_bits;
  q.lo = (uint32_t)(127 + e_lo) << sub_bits;
  q.hi = ((uint32_t)(127 + e_hi + 1) << sub_bits) - 1u;
  q.nm = (e_hi - e_lo + 1) << sub_bits;
  q.nb = 2 * q.nm + 1;
  return true;
}

// workspace of taco_tensor_stats: one record per work item, then (on a 64-byte boundary) each item's nb bucket counts
struct MsWs {
  MsRec* recs;
  uint32_t* part;
  int64_t bytes;
};
MsWs ms_ws(void* ws, int n_items, int nb) {
  WsCarver c(ws);
  MsWs w;
  w.recs = c.take<MsRec>(n_items);
  w.part = c.take<uint32_t>((int64_t)n_items * nb, 64);
  c.take<char>(64);   // slack, for nothing: a base that is not 8-byte aligned is refused.  Callers size buffers with it.
  w.bytes = c.bytes;
  return w;
}

}  // namespace

extern "C" int64_t taco_tensor_stats_plan_bytes(const int64_t* segments, int n) {
  if (!segments || n < 1 || n > TACO_STATS_MAX_SEGMENTS) return TACO_EINVAL;
  const int64_t items = ms_count_items(segments, n, -1);
  if (items < 0 || items > 0x7fffffff) return TACO_EINVAL;
  return (int64_t)sizeof(MsHeader) + n * (int64_t)sizeof(MsSeg) + items * (int64_t)sizeof(MsItem);
}

extern "C" int taco_tensor_stats_plan(const int64_t* segments, int n, int64_t base_floats, void* plan, int64_t plan_bytes,
                                      int32_t* n_items) {
  TACO_REQUIRE(segments && plan && n_items, "tensor_stats: segments, plan or n_items is NULL");
  TACO_REQUIRE(n >= 1 && n <= TACO_STATS_MAX_SEGMENTS, "tensor_stats: n=%d segments, must be in 1..%d", n, TACO_STATS_MAX_SEGMENTS);
  TACO_REQUIRE(base_floats >= 0, "tensor_stats: base_floats=%lld is negative", (long long)base_floats);
  for (int i = 0; i < n; ++i) {
    const int64_t off = segments[2 * i], size = segments[2 * i + 1];
    TACO_REQUIRE(off >= 0 && size >= 0 && off <= MS_MAX_SIZE && size <= MS_MAX_SIZE && off + size <= base_floats,
                 "tensor_stats: segment %d = (offset %lld, size %lld) is outside [0, %lld)", i, (long long)off, (long long)size,
                 (long long)base_floats);
  }
  const int64_t items = ms_count_items(segments, n, base_floats);
  TACO_REQUIRE(items >= 0 && items <= 0x7fffffff, "tensor_stats: %lld work items are more than one plan holds", (long long)items);
  const int64_t need = (int64_t)sizeof(MsHeader) + n * (int64_t)sizeof(MsSeg) + items * (int64_t)sizeof(MsItem);
  TACO_REQUIRE(plan_bytes >= need, "tensor_stats: plan_bytes=%lld, the plan needs %lld", (long long)plan_bytes, (long long)need);
  char* out = static_cast<char*>(plan);
  const MsHeader hd = {MS_MAGIC, n, items, base_floats};
  memcpy(out, &hd, sizeof(hd));
  char* so = out + sizeof(MsHeader);
  char* io = so + n * sizeof(MsSeg);
  int64_t at = 0;
  for (int i = 0; i < n; ++i) {
    const MsSeg sg = {segments[2 * i], segments[2 * i + 1], at, ms_chunks(segments[2 * i], segments[2 * i + 1])};
    memcpy(so + i * sizeof(MsSeg), &sg, sizeof(sg));
    for (int64_t c = 0; c < sg.chunks; ++c) {
      const MsItem it = {i, (int32_t)c};
      memcpy(io + (at + c) * sizeof(MsItem), &it, sizeof(it));
    }
    at += sg.chunks;
  }
  *n_items = (int32_t)items;
  return TACO_OK;
}

extern "C" int64_t taco_tensor_stats_workspace_bytes(int n, int n_items, int nb) {
  if (n < 1 || n > TACO_STATS_MAX_SEGMENTS || n_items < 0 || nb < 3 || nb > TACO_STATS_MAX_BINS || !(nb & 1)) return TACO_EINVAL;
  return ms_ws(nullptr, n_items, nb).bytes;
}

extern "C" int taco_tensor_stats(const float* base, const void* plan_dev, const void* plan_header, int n, int n_items, int e_lo,
                                 int e_hi, int sub_bits, int64_t* counts, double* moments, int64_t* hist, void* workspace,
                                 void* stream) {
  TACO_REQUIRE(base && plan_dev && plan_header && counts && moments && hist && workspace,
               "tensor_stats: base, plan_dev, plan_header, counts, moments, hist or workspace is NULL");
  TACO_REQUIRE(n >= 1 && n <= TACO_STATS_MAX_SEGMENTS, "tensor_stats: n=%d segments, must be in 1..%d", n, TACO_STATS_MAX_SEGMENTS);
  TACO_REQUIRE(n_items >= 0, "tensor_stats: n_items=%d is negative", n_items);
  MsBuckets q;
  TACO_REQUIRE(ms_buckets(e_lo, e_hi, sub_bits, q),
               "tensor_stats: buckets e_lo=%d e_hi=%d sub_bits=%d, need -126 <= e_lo <= e_hi <= 127 and sub_bits in 0..3", e_lo, e_hi,
               sub_bits);
  MsHeader hd;
  memcpy(&hd, plan_header, sizeof(hd));
  TACO_REQUIRE(hd.magic == MS_MAGIC && hd.n == n && hd.n_items == n_items,
               "tensor_stats: the plan's header (n %lld, n_items %lld) does not match n=%d, n_items=%d", (long long)hd.n,
               (long long)hd.n_items, n, n_items);
  TACO_REQUIRE((reinterpret_cast<uintptr_t>(base) & 15) == 0, "tensor_stats: base is not 16-byte aligned");
  TACO_REQUIRE((reinterpret_cast<uintptr_t>(plan_dev) & 7) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
               "tensor_stats: plan_dev or workspace is not 8-byte aligned");
  hipStream_t s = as_stream(stream);
  const char* pd = static_cast<const char*>(plan_dev);
  const MsSeg* segs = reinterpret_cast<const MsSeg*>(pd + sizeof(MsHeader));
  const MsItem* items = reinterpret_cast<const MsItem*>(pd + sizeof(MsHeader) + n * sizeof(MsSeg));
  const MsWs w = ms_ws(workspace, n_items, q.nb);
  MsRec* recs = w.recs;
  uint32_t* part = w.part;
  if (n_items > 0)
    TACO_KLAUNCH(stats_items_kernel, dim3(cdiv(n_items, MS_WAVES)), dim3(MS_T), MS_WAVES * q.nb * sizeof(uint32_t), s, base, segs,
                 items, n_items, q, recs, part);
  const int tiles = cdiv(q.nb, MS_BINS);
  TACO_KLAUNCH(stats_fold_kernel, dim3(n, tiles + 1), dim3(MS_FT), 0, s, segs, q.nb, recs, part, counts, moments, hist, tiles);
  TACO_LAUNCH_CHECK("tensor_stats");
  return TACO_OK;
}
