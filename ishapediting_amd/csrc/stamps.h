// In-kernel time stamps (cdna_hip_programming.md 7, In-kernel stamps): s_memtime of one wave per workgroup at the phase
// boundaries of a kernel, written into a buffer of their own.  Diagnostic builds only (-DISHAP_STAMPS: tools/bench_igemm.hip
// for IG_STAMP, tools/experiments/persist_chain.hip for GN_STAMP; both define the buffer pointers); in the library both
// macros expand to nothing.
#pragma once

#ifdef ISHAP_STAMPS
extern __device__ unsigned long long* g_ig_stamps;      // [workgroup][16]
extern __device__ unsigned long long* g_gn_stamps;      // [workgroup][8]
// the implicit-GEMM kernels: the wave(s) for which `cond` holds
#define IG_STAMP(slot, cond)                                                                                   \
  do {                                                                                                         \
    if (cond) {                                                                                                \
      unsigned long long t_;                                                                                   \
      __builtin_amdgcn_sched_barrier(0);                                                                       \
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                              \
      __builtin_amdgcn_sched_barrier(0);                                                                       \
      if ((threadIdx.x & 63) == 0)                                                                             \
        g_ig_stamps[(size_t)(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z)) * 16 + (slot)] = t_; \
    }                                                                                                          \
  } while (0)
// the group-local GroupNorm kernels: thread 0
#define GN_STAMP(k)                                                                                    \
  do {                                                                                                 \
    if (threadIdx.x == 0) {                                                                            \
      unsigned long long t_;                                                                           \
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                      \
      g_gn_stamps[(size_t)(blockIdx.x + gridDim.x * blockIdx.y) * 8 + (k)] = t_;                       \
    }                                                                                                  \
  } while (0)
#else
#define IG_STAMP(slot, cond) do {} while (0)
#define GN_STAMP(k) do {} while (0)
#endif
