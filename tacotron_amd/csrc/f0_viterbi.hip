// f0_viterbi.hip -- a pitch track smoothed across frames (include/taco_hip.h taco_f0_viterbi): up to K candidates per frame out of
// the autocorrelation taco_frames_f0 writes, one of them (or "unvoiced") chosen per frame by the best path under costs for pitch
// jumps and voiced / unvoiced switches (Boersma 1993).  No counterpart in the reference.  Two launches inside the one call.
//
// (a) Candidates.  A workgroup of 16 x 32 threads owns 32 consecutive frames of a row (the tile of frames_f0_kernel's pick: the
// frame index is the thread's low five bits, 128 contiguous bytes per lag row); 16 threads per frame each own a contiguous run of at
// most 32 lags.  A thread reads its run with both neighbours once, keeps the candidate flags as a bit mask and the local scores
// v = y - bias in LDS, and the K kept candidates come out of K selection rounds under the total order "larger v first, smaller row
// on equal v": a round takes the best candidate that lies strictly behind the previous round's winner in that order, so nothing has
// to be marked as taken (per round: a scan of the run, one barrier, sixteen partial winners combined by every thread alike).  The
// kept ones are ranked by ascending row (sixteen threads per frame, one per entry) and go to three planes of the workspace,
// (B, F, 16) each: the row index, v, and lg of the row; the slots behind the frame's last candidate get v = -inf and lg = 0, so the
// workspace may arrive with anything in it.  Frames at and behind F_b are neither read nor written.
//
// (b) The path.  One workgroup of 256 threads per row; its first wave walks the chain of F_b dependent steps, the others wait at
// a barrier and help with the outputs.  The 64 lanes are 16 target slots x 4 groups of 4 predecessors (lane = 4 c + g): a lane
// scans its four predecessors in ascending order, the four groups of a target are a quad and combine over two quad_perm DPP moves
// carrying the predecessor's index (larger value, then lower index: the lowest p of the largest difference, as a sequential scan
// from p = 0 with a strict > finds it).  D(f - 1, .) of a lane's predecessors comes from their quads by four bpermutes, the frame's
// maximum over wave_max, the sixteen 4-bit back pointers of a frame are one ballot (lane 4 c + g votes bit g of slot c's pointer)
// and go to LDS as one 64-bit word: 8 bytes per frame, 64 KiB at the cap of 8192 frames.  The records of the next kF0vAhead frames
// are in flight while a step is computed.  Behind the chain one lane walks the back pointers into an LDS copy of the path, and the
// workgroup writes period and strength (the pick's parabola on acf), the zeros behind F_b, and the counts (integer LDS atomics: no
// order dependence).  No float atomics anywhere: the same arguments give the same bits.
#include "frames.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int kF0vFrames = 32;              // frames per workgroup of the candidate kernel
constexpr int kF0vParts = 16;               // threads per frame there
constexpr int kF0vSlots = 16;               // slots per frame in the workspace: TACO_F0_MAX_CAND voiced ones and the unvoiced state
constexpr int kF0vAhead = 4;                // frames in flight per lane of the path wave
constexpr int kF0vPathThreads = 256;
constexpr size_t kF0vLdsBudget = 96 * 1024;
constexpr int kF0vNone = 0x7fffffff;
static_assert(TACO_F0_MAX_CAND + 1 == kF0vSlots, "the unvoiced state is the last of sixteen slots");
static_assert(TACO_F0_MAX_LAGS <= 32 * kF0vParts, "a part's run of lags fits a 32-bit candidate mask");

inline size_t f0v_cand_lds(int L) { return ((size_t)L * kF0vFrames + 6 * kF0vParts * kF0vFrames) * 4; }
inline size_t f0v_path_lds(int F) { return (size_t)F * 8 + (size_t)((F + 7) & ~7); }
inline int64_t f0v_plane(int B, int F) { return (int64_t)B * F * kF0vSlots; }   // elements of one workspace plane

// ---- (a) candidates ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kF0vParts* kF0vFrames) void f0_candidates_kernel(const float* __restrict__ acf, const int32_t* __restrict__ frames,
                                                                             int frames_per_unit, const float* __restrict__ bias,
                                                                             const float* __restrict__ lg, int K, int32_t* __restrict__ ws_i,
                                                                             float* __restrict__ ws_v, float* __restrict__ ws_lg, int L,
                                                                             int F, int ntile) {
  // vt [L][32] | pv [2][16][32] | pi [2][16][32] | keep_v [16][32] | keep_i [16][32]
  extern __shared__ __attribute__((aligned(16))) float f0v_lds[];
  float* vt = f0v_lds;
  float* pv = vt + (size_t)L * kF0vFrames;
  int* pi = reinterpret_cast<int*>(pv + 2 * kF0vParts * kF0vFrames);
  float* keep_v = reinterpret_cast<float*>(pi + 2 * kF0vParts * kF0vFrames);
  int* keep_i = reinterpret_cast<int*>(keep_v + kF0vParts * kF0vFrames);
  const int tile = (int)(blockIdx.x % (uint32_t)ntile), b = (int)(blockIdx.x / (uint32_t)ntile);
  const int Fb = row_frames_uniform(frames, frames_per_unit, b, F);
  const int tid = threadIdx.x, fl = tid & 31, pt = tid >> 5;
  const int f0 = tile * kF0vFrames, f = f0 + fl;
  if (f0 >= Fb) return;   // (uniform) nothing of this tile is ever read
  const bool live = f < Fb;
  const int chunk = (L - 2 + kF0vParts - 1) / kF0vParts;   // <= 32
  const int lo = 1 + pt * chunk, hi = min(lo + chunk, L - 1);
  uint32_t mask = 0;
  if (live && lo < hi) {
    const float* __restrict__ y = acf + (int64_t)b * L * F + f;   // (L F <= 512 * 8192: the offsets below fit 32 bits)
    float ym = y[(lo - 1) * F], y0 = y[lo * F];
    for (int i = lo; i < hi; ++i) {
      const float yp = y[(i + 1) * F];
      if (y0 > ym && y0 >= yp) {
        mask |= 1u << (i - lo);
        vt[i * kF0vFrames + fl] = bias ? y0 - bias[i] : y0;
      }
      ym = y0, y0 = yp;
    }
  }
  // K rounds: the best of the run strictly behind the previous winner (wv, wi) in the order "larger v, then smaller row"
  float wv = 0.f;
  int wi = kF0vNone, kf = 0;   // wi == kF0vNone in front of round 0: everything is eligible
  for (int r = 0; r < K; ++r) {
    float bv = 0.f;
    int bi = kF0vNone;
    for (uint32_t m = mask; m; m &= m - 1) {   // ascending rows: a strict > keeps the smallest row of equal scores
      const int i = lo + __builtin_ctz(m);
      const float v = vt[i * kF0vFrames + fl];
      const bool eligible = wi == kF0vNone || v < wv || (v == wv && i > wi);
      if (eligible && (bi == kF0vNone || v > bv)) bv = v, bi = i;
    }
    float* pvr = pv + (r & 1) * kF0vParts * kF0vFrames;
    int* pir = pi + (r & 1) * kF0vParts * kF0vFrames;
    pvr[pt * kF0vFrames + fl] = bv;
    pir[pt * kF0vFrames + fl] = bi;
    __syncthreads();   // (two buffers: round r + 1 writes the other one, and round r + 2 is behind the next barrier)
    bv = 0.f, bi = kF0vNone;
#pragma unroll
    for (int w = 0; w < kF0vParts; ++w) {   // parts in ascending rows: again a strict >
      const float v = pvr[w * kF0vFrames + fl];
      const int i = pir[w * kF0vFrames + fl];
      if (i != kF0vNone && (bi == kF0vNone || v > bv)) bv = v, bi = i;
    }
    if (bi != kF0vNone) {   // (the same for the sixteen threads of a frame.  A frame out of candidates stays out: nothing lies behind
                            //  its last winner; it runs the remaining rounds for the barriers the other frames of its waves need)
      wv = bv, wi = bi;
      if (pt == 0) keep_v[r * kF0vFrames + fl] = bv, keep_i[r * kF0vFrames + fl] = bi;
      ++kf;
    }
  }
  __syncthreads();
  if (!live) return;
  // entry pt of the kept ones goes to the slot of its rank by row; the threads behind the last entry fill the absent slots
  const int64_t at = ((int64_t)b * F + f) * kF0vSlots;
  if (pt < kf) {
    const int mine = keep_i[pt * kF0vFrames + fl];
    int rank = 0;
    for (int j = 0; j < kf; ++j) rank += keep_i[j * kF0vFrames + fl] < mine ? 1 : 0;
    ws_i[at + rank] = mine;
    ws_v[at + rank] = keep_v[pt * kF0vFrames + fl];
    ws_lg[at + rank] = lg[mine];
  } else {
    ws_i[at + pt] = 0;
    ws_v[at + pt] = -INFINITY;
    ws_lg[at + pt] = 0.f;
  }
}

// ---- (b) the path -----------------------------------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ int f0v_dpp_int(int v) {
  return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xf, 0xf, false);
}
// what a lane holds of one frame: its target slot's score and lg, and lg of the four slots it scans as predecessors one frame later
struct F0vRec {
  float v, lc, lq[4];
};
__device__ __forceinline__ F0vRec f0v_load(const float* __restrict__ wv, const float* __restrict__ wl, int f, int last, int c, int g) {
  const int64_t at = (int64_t)min(f, last) * kF0vSlots;   // frames behind the row are read as its last one (inside the planes, never used)
  F0vRec r;
  r.v = wv[at + c];
  r.lc = wl[at + c];
#pragma unroll
  for (int j = 0; j < 4; ++j) r.lq[j] = wl[at + 4 * g + j];
  return r;
}

__global__ __launch_bounds__(kF0vPathThreads) void f0_path_kernel(const float* __restrict__ acf, const int32_t* __restrict__ frames,
                                                                  int frames_per_unit, int lag_min, int K, float threshold,
                                                                  float jump_cost, float switch_cost, const int32_t* __restrict__ ws_i,
                                                                  const float* __restrict__ ws_v, const float* __restrict__ ws_lg,
                                                                  float* __restrict__ period, float* __restrict__ strength,
                                                                  int32_t* __restrict__ counts, float* __restrict__ score, int L, int F) {
  extern __shared__ __attribute__((aligned(16))) uint64_t f0p_lds[];   // back pointers [F] | the path, a byte per frame [F]
  __shared__ int tally[3];
  __shared__ float total;
  uint64_t* bpw = f0p_lds;
  uint8_t* sl = reinterpret_cast<uint8_t*>(f0p_lds + F);
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Fb = row_frames_uniform(frames, frames_per_unit, b, F);
  period += (int64_t)b * F, strength += (int64_t)b * F, counts += (int64_t)b * 4, score += b;
  ws_i += (int64_t)b * F * kF0vSlots, ws_v += (int64_t)b * F * kF0vSlots, ws_lg += (int64_t)b * F * kF0vSlots;
  if (tid < 3) tally[tid] = 0;
  if (Fb > 0 && tid < 64) {   // (uniform per wave) the chain
    const int lane = tid, c = lane >> 2, g = lane & 3, last = Fb - 1;
    const bool c_voiced = c < K, c_off = c == K;
    // T(p -> c) of the lane's four predecessors where it does not depend on the frame (both voiced: it does)
    float fixedT[4];
    bool both[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int p = 4 * g + j;
      both[j] = p < K && c_voiced;
      fixedT[j] = ((p == K) != c_off) ? switch_cost : 0.f;
    }
    F0vRec ahead[kF0vAhead];
    F0vRec cur = f0v_load(ws_v, ws_lg, 0, last, c, g);
#pragma unroll
    for (int k = 0; k < kF0vAhead; ++k) ahead[k] = f0v_load(ws_v, ws_lg, 1 + k, last, c, g);
    float vc = c_voiced ? cur.v : (c_off ? threshold : -INFINITY);
    float m = wave_max(vc);
    float D = vc - m, sum = m;
    float lq[4] = {cur.lq[0], cur.lq[1], cur.lq[2], cur.lq[3]};
    auto step = [&](const F0vRec& now, int f) {
      float best = 0.f;
      int bp = 4 * g;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float Dp = __shfl(D, 16 * g + 4 * j, 64);   // slot 4 g + j lives in the quad of lanes 4 (4 g + j) ..
        const float T = both[j] ? jump_cost * fabsf(lq[j] - now.lc) : fixedT[j];
        const float x = Dp - T;
        if (j == 0) best = x;
        else if (x > best) best = x, bp = 4 * g + j;   // ascending p and a strict >: the lowest p of equal differences
      }
      // the four groups of the target: larger value, then lower predecessor
      {
        const float ov = dpp_move<0xb1>(best, best);   // quad_perm [1,0,3,2]
        const int op = f0v_dpp_int<0xb1>(bp);
        if (ov > best || (ov == best && op < bp)) best = ov, bp = op;
      }
      {
        const float ov = dpp_move<0x4e>(best, best);   // quad_perm [2,3,0,1]
        const int op = f0v_dpp_int<0x4e>(bp);
        if (ov > best || (ov == best && op < bp)) best = ov, bp = op;
      }
      vc = c_voiced ? now.v : (c_off ? threshold : -INFINITY);
      const float E = best + vc;
      m = wave_max(E);
      D = E - m;
      sum = sum + m;
      const uint64_t word = __ballot((bp >> g) & 1);
      if (lane == 0) bpw[f] = word;
#pragma unroll
      for (int j = 0; j < 4; ++j) lq[j] = now.lq[j];
    };
    int f1 = 1;
    for (; f1 + kF0vAhead <= Fb; f1 += kF0vAhead) {
#pragma unroll
      for (int k = 0; k < kF0vAhead; ++k) {
        const F0vRec now = ahead[k];
        ahead[k] = f0v_load(ws_v, ws_lg, f1 + k + kF0vAhead, last, c, g);
        step(now, f1 + k);
      }
    }
#pragma unroll
    for (int k = 0; k < kF0vAhead - 1; ++k) {   // the last Fb - f1 < kF0vAhead frames: their records are loaded
      if (f1 + k >= Fb) break;                  // (uniform)
      step(ahead[k], f1 + k);
    }
    // the end: the lowest slot of the largest D (slots behind K hold -inf, slot K a finite value)
    float ev = D;
    int ec = c;
    for (int o = 32; o; o >>= 1) {
      const float ov = __shfl_xor(ev, o, 64);
      const int oc = __shfl_xor(ec, o, 64);
      if (ov > ev || (ov == ev && oc < ec)) ev = ov, ec = oc;
    }
    if (lane == 0) {   // (it wrote every back-pointer word itself)
      total = sum;
      int s = min(ec, K);
      for (int f = last; f >= 1; --f) {
        sl[f] = (uint8_t)s;
        s = min((int)((bpw[f] >> (4 * s)) & 15), K);   // (it is at most K; the bounds below do not rest on the table's contents)
      }
      sl[0] = (uint8_t)s;
    }
  }
  __syncthreads();
  int voiced = 0, moved = 0, switches = 0;
  for (int f = tid; f < F; f += kF0vPathThreads) {
    float per = 0.f, str = 0.f;
    if (f < Fb) {
      const int s = sl[f];
      const int64_t at = (int64_t)f * kF0vSlots;
      // the frame's own choice: the lowest slot of the largest local score, slot K scoring the threshold
      float lv = ws_v[at];
      int lc = 0;
      for (int q = 1; q < K; ++q) {
        const float v = ws_v[at + q];
        if (v > lv) lv = v, lc = q;
      }
      if (threshold > lv) lc = K;
      moved += s != lc ? 1 : 0;
      if (f >= 1) switches += ((int)sl[f - 1] == K) != (s == K) ? 1 : 0;
      if (s < K) {
        ++voiced;
        int i = ws_i[at + s];
        i = i < 1 ? 1 : (i > L - 2 ? L - 2 : i);   // (a kept row is in 1 .. L - 2; the reads below do not rest on it)
        const float* __restrict__ y = acf + (int64_t)b * L * F + f;
        const float ym = y[(i - 1) * F], y0 = y[i * F], yp = y[(i + 1) * F];
        const float a = ym - yp;
        const float t = y0 + y0;
        const float d = (ym - t) + yp;
        float delta = 0.f;
        if (d != 0.f) {
          delta = __fdiv_rn(0.5f * a, d);
          delta = delta < -0.5f ? -0.5f : (delta > 0.5f ? 0.5f : delta);
        }
        per = (float)(lag_min - 1 + i) + delta;
        str = y0;
      }
    }
    period[f] = per;
    strength[f] = str;
  }
  if (voiced) atomicAdd(&tally[0], voiced);
  if (moved) atomicAdd(&tally[1], moved);
  if (switches) atomicAdd(&tally[2], switches);
  __syncthreads();
  if (tid == 0) {
    counts[0] = Fb, counts[1] = tally[0], counts[2] = tally[1], counts[3] = tally[2];
    score[0] = Fb > 0 ? total : 0.f;
  }
}

bool f0v_shape_ok(int B, int L, int F, int K) {
  return B > 0 && F > 0 && F <= TACO_STRETCH_MAX_FRAMES && L >= 3 && L <= TACO_F0_MAX_LAGS && K >= 1 && K <= TACO_F0_MAX_CAND;
}

// workspace of taco_f0_viterbi: three planes of candidate records, the rows, the values and the log lags
struct F0vWs {
  int32_t* i;
  float *v, *lg;
  int64_t bytes;
};
F0vWs f0v_ws(void* ws, int B, int F) {
  WsCarver c(ws);
  F0vWs w;
  w.i = c.take<int32_t>(f0v_plane(B, F));
  w.v = c.take<float>(f0v_plane(B, F));
  w.lg = c.take<float>(f0v_plane(B, F));
  w.bytes = c.bytes;
  return w;
}

}  // namespace

extern "C" int64_t taco_f0_viterbi_workspace_bytes(int B, int L, int F, int K) {
  if (!f0v_shape_ok(B, L, F, K)) return TACO_EINVAL;
  return f0v_ws(nullptr, B, F).bytes;
}

extern "C" int taco_f0_viterbi(const float* acf, const int32_t* frames, int frames_per_unit, const float* bias, const float* lg, int lag_min,
                               int lag_max, int K, float threshold, float jump_cost, float switch_cost, float* period, float* strength,
                               int32_t* counts, float* score, void* workspace, int B, int F, void* stream) {
  TACO_REQUIRE(acf, "f0_viterbi: acf is NULL");
  TACO_REQUIRE(lg, "f0_viterbi: lg is NULL");
  TACO_REQUIRE(period, "f0_viterbi: period is NULL");
  TACO_REQUIRE(strength, "f0_viterbi: strength is NULL");
  TACO_REQUIRE(counts, "f0_viterbi: counts is NULL");
  TACO_REQUIRE(score, "f0_viterbi: score is NULL");
  TACO_REQUIRE(workspace, "f0_viterbi: workspace is NULL (the candidate records need taco_f0_viterbi_workspace_bytes bytes)");
  TACO_REQUIRE(B > 0, "f0_viterbi: B=%d must be positive", B);
  TACO_REQUIRE(F > 0 && F <= TACO_STRETCH_MAX_FRAMES, "f0_viterbi: F=%d must be in 1..%d", F, TACO_STRETCH_MAX_FRAMES);
  TACO_REQUIRE(lag_min >= 2 && lag_min <= lag_max, "f0_viterbi: lag_min=%d, lag_max=%d must satisfy 2 <= lag_min <= lag_max", lag_min,
               lag_max);
  const int64_t L64 = (int64_t)lag_max - lag_min + 3;
  TACO_REQUIRE(L64 <= TACO_F0_MAX_LAGS, "f0_viterbi: lag_min=%d .. lag_max=%d are %lld lags with their neighbours, at most %d", lag_min,
               lag_max, (long long)L64, TACO_F0_MAX_LAGS);
  const int L = (int)L64;
  TACO_REQUIRE(K >= 1 && K <= TACO_F0_MAX_CAND, "f0_viterbi: K=%d is outside 1 .. %d", K, TACO_F0_MAX_CAND);
  TACO_REQUIRE(threshold == threshold && threshold - threshold == 0.f, "f0_viterbi: threshold=%g must be finite", (double)threshold);
  TACO_REQUIRE(jump_cost >= 0.f && jump_cost - jump_cost == 0.f, "f0_viterbi: jump_cost=%g must be finite and not negative",
               (double)jump_cost);   // (NaN fails the first comparison)
  TACO_REQUIRE(switch_cost >= 0.f && switch_cost - switch_cost == 0.f, "f0_viterbi: switch_cost=%g must be finite and not negative",
               (double)switch_cost);
  TACO_REQUIRE(frames_per_unit >= 1, "f0_viterbi: frames_per_unit=%d must be >= 1", frames_per_unit);
  const uint64_t row = (uint64_t)B * F * 4, abytes = row * (uint64_t)L;
  TACO_REQUIRE(!bytes_meet(period, row, acf, abytes), "f0_viterbi: period overlaps acf");
  TACO_REQUIRE(!bytes_meet(strength, row, acf, abytes), "f0_viterbi: strength overlaps acf");
  TACO_REQUIRE(!bytes_meet(counts, (uint64_t)B * 16, acf, abytes), "f0_viterbi: counts overlaps acf");
  TACO_REQUIRE(!bytes_meet(score, (uint64_t)B * 4, acf, abytes), "f0_viterbi: score overlaps acf");
  const int ntile = cdiv(F, kF0vFrames);
  const int64_t blocks = (int64_t)B * ntile;
  TACO_REQUIRE(blocks <= 0x7fffffff, "f0_viterbi: B=%d x F=%d needs more than 2^31 workgroups", B, F);
  const size_t cand_lds = f0v_cand_lds(L), path_lds = f0v_path_lds(F);
  static DynSmemOnce cand_raised, path_raised;
  if (!ensure_dyn_smem(cand_raised, reinterpret_cast<const void*>(f0_candidates_kernel), kF0vLdsBudget) ||
      !ensure_dyn_smem(path_raised, reinterpret_cast<const void*>(f0_path_kernel), kF0vLdsBudget)) {
    taco_set_error("f0_viterbi: cannot raise the dynamic LDS limit to %zu bytes", kF0vLdsBudget);
    return TACO_ELAUNCH;
  }
  hipStream_t s = as_stream(stream);
  const F0vWs w = f0v_ws(workspace, B, F);
  int32_t* ws_i = w.i;
  float *ws_v = w.v, *ws_lg = w.lg;
  TACO_KLAUNCH(f0_candidates_kernel, dim3((unsigned)blocks), dim3(kF0vParts * kF0vFrames), cand_lds, s, acf, frames, frames_per_unit, bias, lg,
               K, ws_i, ws_v, ws_lg, L, F, ntile);
  TACO_KLAUNCH(f0_path_kernel, dim3((unsigned)B), dim3(kF0vPathThreads), path_lds, s, acf, frames, frames_per_unit, lag_min, K, threshold,
               jump_cost, switch_cost, ws_i, ws_v, ws_lg, period, strength, counts, score, L, F);
  TACO_LAUNCH_CHECK("f0_viterbi");
  return TACO_OK;
}
