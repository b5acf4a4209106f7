// Exact squared Euclidean distance transform of a byte grid [n0][n1][n2], n2 fastest (include/ishap.h: ishap_edt).
//
// The transform is separable: one pass per measured axis, each the 1-D min-plus  out[i] = min_j (i - j)^2 + f[j]  along its
// axis.  The first pass reads the seed bytes as f = 0 / EDT_INF, every later one the int32 result of the pass before; the passes
// alternate between `dist2` and the caller's scratch so that the last one lands in `dist2`.  Everything is int32: the largest
// sum formed is EDT_INF + 1023^2 < 2^31, no floating point, no atomics, every output written by exactly one thread.
//
// The search for the minimum walks outwards from j = i, d = 1, 2, ..., and stops as soon as d^2 >= the best value so far: j = i
// is itself a candidate, so nothing farther along the line can win (the exact prune |i - j| <= floor(sqrt(best)), without a
// square root, and tightening as the best value falls).  It also stops at the line's first and last finite entry, found in one
// sweep before: a line without a seed costs nothing more, which is what keeps a sparse 1024^3 call bounded.  So the work per
// output is the distance to the set, small wherever the set is near.
//
//   edt_col_kernel  passes along axis 0 and axis 1.  A thread per line, consecutive threads on consecutive n2: every load and
//                   store of a wave is one coalesced row segment, and a lane walks its own line with the axis' stride.  A lane
//                   keeps four integers, no array: no private segment.
//   edt_row_kernel  the pass along axis 2.  A wave per line: the line goes to LDS with coalesced loads (4 KiB per wave at most),
//                   lane l then forms outputs l, l + 64, ...; neighbouring lanes read neighbouring LDS words.
// Once per edit; nothing here is on the per-step path.
#include "../../include/ishap.h"
#include "edt.h"

namespace {
constexpr int ET = 256;
constexpr int EDT_WAVES = ET / 64;

template <bool FIRST>
__device__ __forceinline__ int edt_load(const void* __restrict__ src, long long i, unsigned mask, int invert) {
  if (FIRST) {
    const bool set = (static_cast<const unsigned char*>(src)[i] & mask) != 0;
    return set != (invert != 0) ? 0 : EDT_INF;
  }
  return static_cast<const int*>(src)[i];
}

// T lines; line t starts at (t / inner) * outer_stride + t % inner and steps by `step`, L entries.  Axis 0: inner = T = n1 n2,
// step = n1 n2 (the start is t itself); axis 1: inner = n2, outer_stride = n1 n2, step = n2.
template <bool FIRST>
__global__ __launch_bounds__(ET) void edt_col_kernel(const void* __restrict__ src, unsigned mask, int invert, long long T, long long inner,
                                                     long long outer_stride, long long step, int L, int* __restrict__ out) {
  const long long t = (long long)blockIdx.x * ET + threadIdx.x;
  if (t >= T) return;
  const long long base = (t / inner) * outer_stride + t % inner;
  int lo = L, hi = -1;                                         // the line's first and last finite entry
  for (int j = 0; j < L; ++j)
    if (edt_load<FIRST>(src, base + j * step, mask, invert) < EDT_INF) {
      lo = min(lo, j);
      hi = j;
    }
  for (int i = 0; i < L; ++i) {
    int best = edt_load<FIRST>(src, base + i * step, mask, invert);
    const int dmax = max(i - lo, hi - i);
    for (int d = max(1, max(lo - i, i - hi)); d <= dmax && d * d < best; ++d) {      // nothing finite nearer than that
      if (i - d >= lo) best = min(best, edt_load<FIRST>(src, base + (i - d) * step, mask, invert) + d * d);
      if (i + d <= hi) best = min(best, edt_load<FIRST>(src, base + (i + d) * step, mask, invert) + d * d);
    }
    out[base + i * step] = best;
  }
}

// lines of L <= EDT_MAX_AXIS contiguous entries, a wave each
template <bool FIRST>
__global__ __launch_bounds__(ET) void edt_row_kernel(const void* __restrict__ src, unsigned mask, int invert, long long lines, int L,
                                                     int* __restrict__ out) {
  __shared__ int f[EDT_WAVES][EDT_MAX_AXIS];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long line = (long long)blockIdx.x * EDT_WAVES + w;
  const bool live = line < lines;                              // wave-uniform; no early return: the barrier below is for all
  int lo = L, hi = -1;
  if (live)
    for (int j = lane; j < L; j += 64) {
      const int v = edt_load<FIRST>(src, line * L + j, mask, invert);
      f[w][j] = v;
      if (v < EDT_INF) {
        lo = min(lo, j);
        hi = max(hi, j);
      }
    }
  for (int m = 32; m >= 1; m >>= 1) {
    lo = min(lo, __shfl_xor(lo, m));
    hi = max(hi, __shfl_xor(hi, m));
  }
  __syncthreads();
  if (!live) return;
  for (int i = lane; i < L; i += 64) {
    int best = f[w][i];
    const int dmax = max(i - lo, hi - i);
    for (int d = max(1, max(lo - i, i - hi)); d <= dmax && d * d < best; ++d) {      // nothing finite nearer than that
      if (i - d >= lo) best = min(best, f[w][i - d] + d * d);
      if (i + d <= hi) best = min(best, f[w][i + d] + d * d);
    }
    out[line * L + i] = best;
  }
}

template <bool FIRST>
void edt_pass(const void* src, unsigned mask, int invert, int n0, int n1, int n2, int axis, int* out, hipStream_t s) {
  const long long n12 = (long long)n1 * n2, n = n12 * n0;
  if (axis == 2) {
    const long long lines = n / n2;
    hipLaunchKernelGGL(edt_row_kernel<FIRST>, dim3((unsigned)((lines + EDT_WAVES - 1) / EDT_WAVES)), dim3(ET), 0, s, src, mask, invert,
                       lines, n2, out);
    return;
  }
  const int L = axis == 0 ? n0 : n1;
  const long long T = n / L;
  const long long inner = axis == 0 ? T : (long long)n2, outer_stride = axis == 0 ? 0 : n12, step = axis == 0 ? n12 : (long long)n2;
  hipLaunchKernelGGL(edt_col_kernel<FIRST>, dim3((unsigned)((T + ET - 1) / ET)), dim3(ET), 0, s, src, mask, invert, T, inner, outer_stride,
                     step, L, out);
}

int edt_passes(int axes) { return (axes & 1) + ((axes >> 1) & 1) + ((axes >> 2) & 1); }
}  // namespace

long long edt_scratch_bytes(int n0, int n1, int n2, int axes) {
  if (n0 < 1 || n1 < 1 || n2 < 1 || axes < 1 || axes > 7) return -1;
  const long long n = (long long)n0 * n1 * n2;
  if ((long long)n0 * n1 >= (1ll << 31) || n >= (1ll << 31)) return -1;
  const int len[3] = {n0, n1, n2};
  for (int a = 0; a < 3; ++a)
    if (((axes >> a) & 1) && len[a] > EDT_MAX_AXIS) return -1;
  return edt_passes(axes) > 1 ? (long long)align_up((size_t)(4 * n), 256) : 256;      // the other buffer of the alternation
}

int edt_launch(const unsigned char* seeds, unsigned mask, int n0, int n1, int n2, int axes, int invert, int* dist2, void* scratch,
               hipStream_t s) {
  const int np = edt_passes(axes);
  const void* src = seeds;
  for (int a = 0, k = 0; a < 3; ++a) {
    if (!((axes >> a) & 1)) continue;
    int* dst = ((np - 1 - k) & 1) ? (int*)scratch : dist2;
    if (k == 0) edt_pass<true>(src, mask, invert, n0, n1, n2, a, dst, s);
    else edt_pass<false>(src, 0u, 0, n0, n1, n2, a, dst, s);
    src = dst;
    ++k;
  }
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" long long ishap_edt_scratch_bytes(int n0, int n1, int n2, int axes) { return edt_scratch_bytes(n0, n1, n2, axes); }

extern "C" int ishap_edt(const unsigned char* seeds, int n0, int n1, int n2, int axes, int invert, int* dist2, void* scratch,
                         long long scratch_bytes, void* stream) {
  static_assert(ISHAP_EDT_INF == EDT_INF, "ISHAP_EDT_INF");
  ISHAP_REQUIRE(axes >= 1 && axes <= 7, "edt: axes is a mask of the measured axes, 1..7");
  ISHAP_REQUIRE(invert == 0 || invert == 1, "edt: invert is 0 or 1");
  const long long need = edt_scratch_bytes(n0, n1, n2, axes);
  ISHAP_REQUIRE(need > 0, "edt: sizes must be >= 1, every measured axis <= 1024 and n0 * n1 * n2 < 2^31");
  ISHAP_REQUIRE(seeds && dist2 && scratch, "edt: null argument");
  ISHAP_REQUIRE(scratch_bytes >= need, "edt: scratch smaller than ishap_edt_scratch_bytes(n0, n1, n2, axes)");
  ISHAP_REQUIRE(((unsigned long long)scratch & 3ull) == 0 && ((unsigned long long)dist2 & 3ull) == 0, "edt: dist2 and scratch must be 4-byte aligned");
  const long long n = (long long)n0 * n1 * n2;
  const char *s0 = (const char*)seeds, *d0 = (const char*)dist2;
  ISHAP_REQUIRE(s0 + n <= d0 || d0 + 4 * n <= s0, "edt: seeds and dist2 must not alias");
  return edt_launch(seeds, 0xffu, n0, n1, n2, axes, invert, dist2, scratch, (hipStream_t)stream);
}
