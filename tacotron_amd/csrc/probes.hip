// probes.hip -- three machine probes behind debug entry points (include/taco_hip.h taco_debug_spin, taco_debug_clock_probe,
// taco_debug_fabric_probe): a stand-in for a communication kernel, the shader clock under a latency-bound load, and the fabric's
// round trips.  None is on the train step's or the synthesis path; tools and tests call them.
#include "common.h"
#include "kernels.h"

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
