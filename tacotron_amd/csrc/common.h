// common.h -- shared host/device helpers for libtaco_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/taco_hip.h"
#include "switches.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- host-side error plumbing -----------------------------------------------------------------------------
void taco_set_error(const char* fmt, ...);

#define TACO_REQUIRE(cond, ...)        \
  do {                                 \
    if (!(cond)) {                     \
      taco_set_error(__VA_ARGS__);     \
      return TACO_EINVAL;              \
    }                                  \
  } while (0)

#define TACO_LAUNCH_CHECK(what)                                             \
  do {                                                                      \
    hipError_t e__ = hipGetLastError();                                     \
    if (e__ != hipSuccess) {                                                \
      taco_set_error("%s: %s", what, hipGetErrorString(e__));               \
      return TACO_ELAUNCH;                                                  \
    }                                                                       \
  } while (0)

#define TACO_TRY(expr)          \
  do {                          \
    int rc__ = (expr);          \
    if (rc__ != TACO_OK) return rc__; \
  } while (0)

// Model constants (reference Config, tacotron.py:12-33; CBHG widths ops.py:48-49, tacotron.py:131,147).
constexpr int kEmbed = 256;
constexpr int kPre1 = 256;
constexpr int kPre2 = 128;
constexpr int kCb = 128;    // CBHG channel width / GRU units
constexpr int kAtt = 256;   // attention_units
constexpr int kDec = 256;   // decoder_units
constexpr int kMel = 80;
constexpr int kFft = 1025;
constexpr float kBnEps = 1e-3f;

// ---- device math ------------------------------------------------------------------------------------------
__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float tanh_f(float x) {
  // 2/(1+e^-2x) - 1 : absolute error ~1e-7, saturates cleanly (e^-2x -> inf gives -1, -> 0 gives 1).
  return 2.0f / (1.0f + expf(-2.0f * x)) - 1.0f;
}

// Attention inner loops only: tanh on the hardware exp / rcp units (v_exp_f32, v_rcp_f32; ~1 ulp each), absolute error
// ~2e-7 -- 51 K tanh per row-step make the IEEE-division version the largest VALU cost of the attention phases.
__device__ __forceinline__ float sigmoid_fast(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float tanh_fast(float x) {
  return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(2.0f * x));
}

// Wave64 reductions on the DPP path (gfx9 row_ror / row_bcast: plain VALU moves, no LDS-crossbar ds_bpermute as __shfl_xor
// uses): quad_perm swaps + row_ror 4/8 leave every lane of a 16-lane row with the row total; row_bcast:15 / :31 then fold the
// four rows so lanes 48..63 hold the wave total, which v_readlane broadcasts.  ~6 VALU ops instead of 6 dependent shuffles.
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ float dpp_move(float old, float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ float wave_sum(float v) {
  v += dpp_move<0xb1>(0.f, v);          // quad_perm [1,0,3,2]
  v += dpp_move<0x4e>(0.f, v);          // quad_perm [2,3,0,1]
  v += dpp_move<0x124>(0.f, v);         // row_ror:4
  v += dpp_move<0x128>(0.f, v);         // row_ror:8
  v += dpp_move<0x142, 0xa>(0.f, v);    // row_bcast:15 -> rows 1,3
  v += dpp_move<0x143, 0xc>(0.f, v);    // row_bcast:31 -> rows 2,3
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ float wave_max(float v) {
  v = fmaxf(v, dpp_move<0xb1>(v, v));
  v = fmaxf(v, dpp_move<0x4e>(v, v));
  v = fmaxf(v, dpp_move<0x124>(v, v));
  v = fmaxf(v, dpp_move<0x128>(v, v));
  v = fmaxf(v, dpp_move<0x142, 0xa>(v, v));
  v = fmaxf(v, dpp_move<0x143, 0xc>(v, v));
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// Counter-based random bits (the Bernoulli masks, the device phases of taco_griffinlim_rows): draw i of a seed is the output
// function of the splitmix64 generator on seed * 0xD1342543DE82EF95 + i, in 64-bit wrap-around arithmetic
__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
__device__ __forceinline__ uint64_t counter_hash(uint64_t seed, uint64_t i) { return splitmix64(seed * 0xD1342543DE82EF95ull + i); }

// Workgroup barrier for LDS-only communication: waits for this wave's LDS traffic (lgkmcnt) but NOT for its outstanding
// global loads/stores (vmcnt), unlike __syncthreads(), so prefetch loads and stash stores stay in flight across it.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__device__ __forceinline__ float apply_act(float x, int act) {
  switch (act) {
    case TACO_ACT_RELU: return fmaxf(x, 0.0f);
    case TACO_ACT_SIGMOID: return sigmoid_f(x);
    case TACO_ACT_TANH: return tanh_f(x);
    default: return x;
  }
}

// hipFuncAttributeMaxDynamicSharedMemorySize is a property of the (function, DEVICE) pair: cache the "already raised" fact per
// device, not per process (a second GPU used by the same process would otherwise launch without it and fail).  `done` is the
// call site's own static table.
struct DynSmemOnce {
  bool ok[32] = {};
};
static inline bool ensure_dyn_smem(DynSmemOnce& done, const void* func, size_t bytes) {
  if (bytes <= 64 * 1024) return true;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  if (dev >= 0 && dev < 32 && done.ok[dev]) return true;
  if (hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return false;
  if (dev >= 0 && dev < 32) done.ok[dev] = true;
  return true;
}

// ---- argument checks of the op-level debug doors (taco_debug_bigru_*, taco_debug_highway_stack_*, taco_debug_prenet_*) ----
// Every operand of a call as (name, pointer, bytes, written by the call, may be null).  A missing operand, or an output whose
// bytes meet those of any other operand, is refused by name before anything is enqueued.
struct DoorOperands {
  struct Op { char name[24]; const void* p; size_t bytes; bool out, optional; };
  static constexpr int kMax = 192;   // (taco_debug_transpose_batch: 2 operands for each of kMaxTransposeBatch = 96 jobs)
  Op ops[kMax];
  int n = 0;
  bool overflow = false;   // an operand that did not fit: check() refuses the call instead of leaving it unchecked
  void add(const void* p, size_t bytes, bool out, bool optional, const char* fmt, int idx = 0) {
    if (n >= kMax) { overflow = true; return; }
    Op& o = ops[n++];
    snprintf(o.name, sizeof(o.name), fmt, idx);
    o.p = p; o.bytes = bytes; o.out = out; o.optional = optional;
  }
  void in(const void* p, size_t bytes, const char* fmt, int idx = 0) { add(p, bytes, false, false, fmt, idx); }
  void in_opt(const void* p, size_t bytes, const char* fmt, int idx = 0) { add(p, bytes, false, true, fmt, idx); }
  void out(const void* p, size_t bytes, const char* fmt, int idx = 0) { add(p, bytes, true, false, fmt, idx); }
  void out_opt(const void* p, size_t bytes, const char* fmt, int idx = 0) { add(p, bytes, true, true, fmt, idx); }
  int check(const char* who) const {
    TACO_REQUIRE(!overflow, "%s: more than %d operands to check", who, kMax);
    for (int i = 0; i < n; ++i)
      TACO_REQUIRE(ops[i].p || ops[i].optional, "%s: %s is null", who, ops[i].name);
    for (int i = 0; i < n; ++i) {
      if (!ops[i].out || !ops[i].p) continue;
      const char* o0 = static_cast<const char*>(ops[i].p);
      for (int j = 0; j < n; ++j) {
        if (j == i || !ops[j].p || (ops[j].out && j < i)) continue;   // (a pair of outputs is reported once)
        const char* i0 = static_cast<const char*>(ops[j].p);
        TACO_REQUIRE(!(o0 < i0 + ops[j].bytes && i0 < o0 + ops[i].bytes), "%s: %s may not overlap %s", who, ops[i].name, ops[j].name);
      }
    }
    return TACO_OK;
  }
};

// bytes of a (rows, cols) operand with row pitch ld, and the size limits of the GEMM-form doors (gemm.hip, gemm2.hip, elementwise.hip)
static inline size_t door_span(int64_t rows, int64_t cols, int64_t ld) { return (size_t)((rows - 1) * ld + cols) * sizeof(float); }
constexpr int kDoorMaxRows = 1 << 22, kDoorMaxCols = 1 << 14;

// ---- workspaces of the auxiliary entry points ---------------------------------------------------------------------------------
// One walk over a workspace serves both its size function (built from nullptr: the walk only counts) and its entry point (built
// from the caller's pointer: the walk hands out the arrays), so the two cannot disagree.  take<T>(count, align) returns the next
// array, at an offset from the base that is a multiple of align, and advances.  base_align > 1 first rounds the caller's pointer
// up to it; the bytes that costs are not counted, the layout's slack term pays for them.
struct WsCarver {
  char* base;          // nullptr: count only
  int64_t bytes = 0;   // consumed so far
  explicit WsCarver(void* ws, uintptr_t base_align = 1)
      : base(reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(ws) + base_align - 1) / base_align * base_align)) {}
  template <class T>
  T* take(int64_t count, int64_t align = alignof(T)) {
    bytes = (bytes + align - 1) / align * align;
    T* p = base ? reinterpret_cast<T*>(base + bytes) : nullptr;
    bytes += count * (int64_t)sizeof(T);
    return p;
  }
};

// whether the byte ranges [a, a + abytes) and [b, b + bbytes) meet: the overlap refusals of every entry point outside DoorOperands
static inline bool bytes_meet(const void* a, uint64_t abytes, const void* b, uint64_t bbytes) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + bbytes && b0 < a0 + abytes;
}

static inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }
static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// TACO_DETERMINISTIC=1: every reduction that is otherwise combined with fp32 atomics (split-M weight gradients, the K-way conv
// bank input gradient, BN / bias column sums, the embedding scatter) runs in a fixed order instead -- slower, but two runs of
// the same step give bit-identical gradients (needed to bisect a training divergence).  Read on every call.
static inline bool taco_deterministic() { return sw_on<SW_DETERMINISTIC>(); }
