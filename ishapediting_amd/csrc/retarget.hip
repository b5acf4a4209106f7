// Closed-loop drag: re-aim the loss at the tracked handles and rebuild what it derives from its targets.  DragGAN supervises a
// short move from each handle's CURRENT position towards the target, tracks, and repeats; the tracker (track.hip) supplies the
// current positions as integer voxel offsets K, this file turns them into the step's goals.  The definition is DESIGN.md 5.2m.
//
// One launch per tracked step, a workgroup of 1024 threads per edit:
//   1. re-aim: a thread per handle forms goal, remaining and arrived in double (contraction off) and writes them;
//   2. the edit's three plane bitmaps are cleared in LDS (3*W*W bytes of dynamic LDS);
//   3. they are marked with LDS atomicOr under drag_touch_marks (drag.h), the rule the setup's global-memory kernel applies, on
//      sources and GOALS -- as if the setup had been given targets = goals;
//   4. the bitmaps leave for `touched` in 16-byte stores while the texels with bit 0 clear are counted; one reduction gives
//      nmask[e] and done[e].
// No global atomics, no memset, no float atomics: every output is a plain store of a value that does not depend on the order in
// which threads ran, so a retarget is bitwise repeatable and an edit's outputs do not depend on the edits beside it.  gfx, acc
// (left zero by every loss call) and chw (independent of the handles) are not touched.
#include "retarget.h"
#include <cmath>

// goal, remaining and arrived of one handle: DESIGN.md 5.2m, every operation in double, in the order written there
__device__ __forceinline__ void retarget_reaim(const float* __restrict__ src, const float* __restrict__ tgt, const int* __restrict__ K,
                                               float voxel, float step_f, float arrive_f, float (&goal)[3], float* remaining, int* arrived) {
#pragma clang fp contract(off)
  const double vx = (double)voxel, step = (double)step_f;
  const float s0 = src[0], s1 = src[1], s2 = src[2], t0 = tgt[0], t1 = tgt[1], t2 = tgt[2];
  const int k0 = K[0], k1 = K[1], k2 = K[2];
  const double r0 = ((double)t0 - (double)s0) / vx - (double)k0;
  const double r1 = ((double)t1 - (double)s1) / vx - (double)k1;
  const double r2 = ((double)t2 - (double)s2) / vx - (double)k2;
  const double d = sqrt((r0 * r0 + r1 * r1) + r2 * r2);
  const bool hold = d <= step;          // within the lead (d = 0 included: no 0 / 0): the target itself, a bit copy
  const float g0 = (float)((double)s0 + vx * ((double)k0 + step * r0 / d));
  const float g1 = (float)((double)s1 + vx * ((double)k1 + step * r1 / d));
  const float g2 = (float)((double)s2 + vx * ((double)k2 + step * r2 / d));
  goal[0] = hold ? t0 : g0;
  goal[1] = hold ? t1 : g1;
  goal[2] = hold ? t2 : g2;
  remaining[0] = (float)d;
  arrived[0] = d <= (double)arrive_f ? 1 : 0;
}

__global__ __launch_bounds__(RETARGET_THREADS) void drag_retarget_kernel(DragBatchArgs b, RetargetArgs q) {
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  extern __shared__ __attribute__((aligned(16))) unsigned char retarget_lds[];   // [3][W][W]: the edit's bitmaps
  __shared__ int red[2 * RETARGET_THREADS / 64];                                 // the reduction scratch
  const int e = blockIdx.x, tid = threadIdx.x;
  const int h0 = b.hoff[e];
  DragArgs a = drag_edit_args(b, e);
  a.targets = q.goals + 3 * h0;               // the rule below reads the goals where the setup reads the targets
  const int nbytes = 3 * a.W * a.W, nwords = nbytes >> 2;     // 3*W*W % 4 == 0 (drag_batch_check)

  // 1. re-aim.  Loads are unconditional at a clamped handle (a thread past the end recomputes the last handle and stores nothing)
  int waiting = 0;                            // handles of this thread that have not arrived
  for (int hb = 0; hb < a.B; hb += RETARGET_THREADS) {       // workgroup-uniform trip count: one trip up to 1024 handles
    const int h = min(hb + tid, a.B - 1), g = h0 + h;
    float goal[3], rem;
    int arr;
    retarget_reaim(a.sources + 3 * h, q.final_targets + 3 * g, q.K + 3 * g, a.voxel, q.step[e], q.arrive[e], goal, &rem, &arr);
    if (hb + tid < a.B) {
      q.goals[3 * g] = goal[0]; q.goals[3 * g + 1] = goal[1]; q.goals[3 * g + 2] = goal[2];
      q.remaining[g] = rem;
      q.arrived[g] = arr;
      waiting += 1 - arr;
    }
  }
  // 2. clear
  unsigned* words = reinterpret_cast<unsigned*>(retarget_lds);
  for (int i = tid; i < nwords; i += RETARGET_THREADS) words[i] = 0u;
  __syncthreads();                            // the goals (global, this workgroup's own stores) and the cleared bitmaps are visible

  // 3. mark: one (handle, plane, source / goal, lattice i, j) tuple per trip, decomposed as drag_batch_touch_kernel does.  Which
  // thread marks which tuple is free: OR commutes.  (Measured and dropped: a wave per (handle, plane, source / goal) that loads
  // the point once and walks its positions without a global load in the trip -- 134 us against 104 us for 16 handles; the trip
  // is bound by its 17 dependent LDS round trips, not by the two loads.)
  const int side = 2 * a.r + 1, per = 3 * 2 * side * side;
  const int total = per * a.B;                // < 2^31: checked by the launcher
  for (int idx = tid; idx < total; idx += RETARGET_THREADS) {
    const int h = idx / per;
    int rem = idx - h * per;
    const int j = rem % side; rem /= side;
    const int i = rem % side; rem /= side;
    const int st = rem % 2;
    const int p = rem / 2;
    // The lattice pitch is a fraction of a texel (a quarter at the real shape), so the 17 marks of nearly every tuple are set
    // already, and 1024 threads' atomics on the same few dozen words serialise: read first (same-address LDS reads broadcast)
    // and OR only what is missing (104 us against 223 us for 16 handles).  Bits are only ever set in this phase, so a stale
    // read costs a redundant OR, never a mark.
    drag_touch_marks(a, p, h, st, i, j, [&](long long o, unsigned bit) {
      unsigned* w = words + (int)(o >> 2);
      const unsigned m = bit << (8 * (int)(o & 3));
      if ((__atomic_load_n(w, __ATOMIC_RELAXED) & m) != m) atomicOr(w, m);
    });
  }
  __syncthreads();

  // 4. store and count.  16-byte stores where the slice allows them (3*W*W % 16 == 0 and an aligned base: every W % 4 == 0)
  const bool vec = (nbytes & 15) == 0 && (reinterpret_cast<unsigned long long>(a.touched) & 15ull) == 0;
  const int nvec = vec ? nbytes >> 4 : 0;
  int untouched = 0;
  auto clear0 = [](unsigned w) { return 4 - __popc(w & 0x01010101u); };       // bytes of w with bit 0 clear
  for (int i = tid; i < nvec; i += RETARGET_THREADS) {
    const u32x4 v = reinterpret_cast<const u32x4*>(retarget_lds)[i];
    reinterpret_cast<u32x4*>(a.touched)[i] = v;
    untouched += (clear0(v[0]) + clear0(v[1])) + (clear0(v[2]) + clear0(v[3]));
  }
  for (int i = 4 * nvec + tid; i < nwords; i += RETARGET_THREADS) {
    const unsigned w = words[i];
    reinterpret_cast<unsigned*>(a.touched)[i] = w;
    untouched += clear0(w);
  }
  for (int o = 32; o > 0; o >>= 1) { untouched += __shfl_xor(untouched, o); waiting += __shfl_xor(waiting, o); }
  if ((tid & 63) == 0) { red[2 * (tid >> 6)] = untouched; red[2 * (tid >> 6) + 1] = waiting; }
  __syncthreads();
  if (tid == 0) {
    int u = 0, w = 0;
#pragma unroll
    for (int k = 0; k < RETARGET_THREADS / 64; ++k) { u += red[2 * k]; w += red[2 * k + 1]; }
    a.nmask[0] = u;
    q.done[e] = w == 0 ? 1 : 0;
  }
}

int drag_retarget_launch(DragBatchArgs& a, const RetargetArgs& q, hipStream_t s) {
  ISHAP_REQUIRE(q.final_targets && q.K && q.goals && q.remaining && q.arrived && q.done, "drag retarget: null argument");
  ISHAP_REQUIRE(a.E >= 1 && a.E <= DRAG_MAX_EDITS, "drag batch: E must be in 1..32");
  for (int e = 0; e < a.E; ++e) {
    ISHAP_REQUIRE(q.step[e] > 0.f, "drag retarget: step must be > 0 (it may be +inf) and not NaN");
    ISHAP_REQUIRE(q.arrive[e] >= 0.f, "drag retarget: arrive must be >= 0 and not NaN");
  }
  ISHAP_REQUIRE(a.base.W > 1 && 3ll * a.base.W * a.base.W <= RETARGET_LDS_BYTES,
                "drag retarget: the three plane bitmaps, 3*W*W bytes, must fit 65536 bytes of LDS (W <= 147)");
  ISHAP_REQUIRE(q.goals != q.final_targets, "drag retarget: the goals buffer must not be the final targets");
  ISHAP_TRY(drag_batch_check(a));
  const long long side = 2ll * a.base.r + 1;
  ISHAP_REQUIRE(a.base.r >= 0 && 6 * side * side * a.hoff[a.E] < (1ll << 31) - RETARGET_THREADS, "drag retarget: too many lattice points");
  ISHAP_REQUIRE((reinterpret_cast<unsigned long long>(a.base.touched) & 3ull) == 0, "drag retarget: touched must be 4-byte aligned");
  const size_t lds = (size_t)3 * a.base.W * a.base.W;
  hipLaunchKernelGGL(drag_retarget_kernel, dim3(a.E), dim3(RETARGET_THREADS), lds, s, a, q);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}
