// Drag guidance: motion-supervision loss on the UNet decoder feature and its gradient.
// Reference: drag_utils.py:141-159 (resize_feat_align: [1,2c,H,W] -> [3, 2*(c//3), H, W]),
// :309-334 (lattices, planar grids, int16 texel ids, complement "mask" sets via Python sets),
// :355-382 (grid_sample bilinear/zeros/align_corners=True of origin at the source lattice and of the
// edited feature at the target lattice; L2 or L1 mean; mask regulariser on untouched texels).
// The reference back-propagates this through autograd; here the gradient w.r.t. the tap is
// produced directly, in the tap's own NHWC layout, ready for the UNet backward pass.
//
// Observation that shrinks the work 2r+1 times: plane xy only sees (x,y) of a lattice point, so the
// (2r+1) lattice points that differ in z are identical terms of the mean.  Each plane therefore has
// B*(2r+1)^2 distinct sample positions with multiplicity (2r+1).  A wave owns one position; lanes run
// over channels, which are contiguous in NHWC (coalesced 2-byte reads, fp32 atomics for the scatter).
//
// One set of kernels: the per-edit device bodies first, then the kernels and launches, which take E edits per call
// (DragBatchArgs).  One edit is the E = 1 call.
#include "drag.h"
#include <cstdlib>

// plane_axes, lattice and bilin_setup (the sampling of every drag kernel, csrc/track.hip included) and drag_touch_marks (the
// touched-texel rule, csrc/retarget.hip included) are in drag.h

// workgroup sum of the per-lane loss terms, then ONE atomic on the accumulator (thousands of same-address atomics
// -- one per wave -- were the whole run time of these kernels)
__device__ __forceinline__ void fx_add(long long* dst, float v, float scale) {
  atomicAdd(reinterpret_cast<unsigned long long*>(dst), (unsigned long long)__float2ll_rn(v * scale));
}
// The 256 lane sums are added in double (fixed order: repeatable bits) and the workgroup's total is rounded ONCE, to the
// accumulator's 2^-24: the loss carries no rounding of this tree.
__device__ __forceinline__ void block_loss_add(float lsum, long long* dst) {
  __shared__ double red[4];
  double v = (double)lsum;
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0)
    atomicAdd(reinterpret_cast<unsigned long long*>(dst),
              (unsigned long long)__double2ll_rn(((red[0] + red[1]) + (red[2] + red[3])) * (double)DRAG_ACC_SCALE));
}

constexpr int DSEG = 5;     // consecutive lattice positions a wave walks
// Motion term.  A wave owns DSEG consecutive positions of one lattice ROW of one (plane, handle) pair and one chunk of 64
// channels, and walks them in order.  The bilinear row pair (y0, y0+1) of the target is the same for the whole row and
// consecutive positions are a fraction of a texel apart, so the scatter of a row lands in a few texel columns: the
// contributions are summed in registers per column and leave as one fixed-point atomic per (column, row) instead of four
// per position (3x fewer 64-bit atomics).  Summation order is fixed, the final
// adds are integer, so edits stay bitwise repeatable.
__device__ __forceinline__ void drag_motion_body(const DragArgs& a, int blk, int nblk) {
  const int side = 2 * a.r + 1;
  const int nchunk = (a.Cc + 63) / 64;
  const int nseg = (side + DSEG - 1) / DSEG;
  const int nrows = 3 * a.B * side * nchunk * nseg;
  const int lane = threadIdx.x & 63;
  const int nwaves = (nblk * blockDim.x) >> 6;
  const float mult = (float)side;
  const float ntot = 3.f * (float)a.Cc * (float)a.B * (float)side * (float)side * (float)side;
  float lsum = 0.f;
  for (int wave = (blk * blockDim.x + threadIdx.x) >> 6; wave < nrows; wave += nwaves) {
    const int seg = wave % nseg;
    const int cchunk = (wave / nseg) % nchunk;
    const int j = (wave / (nseg * nchunk)) % side;           // lattice index along the row axis
    const int b = (wave / (nseg * nchunk * side)) % a.B;
    const int p = wave / (nseg * nchunk * side * a.B);
    int ac, ar;
    plane_axes(p, ac, ar);
    const int c = cchunk * 64 + lane;
    const bool live = c < a.Cc;
    const int ch = live ? a.chmap[p * a.Cc + c] : 0;
    const float su = a.sources[b * 3 + ac], sv = lattice(a.sources[b * 3 + ar], a.voxel, j - a.r);
    const float tu = a.targets[b * 3 + ac], tv = lattice(a.targets[b * 3 + ar], a.voxel, j - a.r);
    float a00 = 0.f, a01 = 0.f, a10 = 0.f, a11 = 0.f;     // [row y0 / y0+1][column xcur / xcur+1]
    int xcur = 0, ycur = 0;
    bool open = false;
    auto flush_col = [&](int x, float v0, float v1) {
      if (!live || x < 0 || x >= a.W) return;
      if (ycur >= 0 && ycur < a.W) fx_add(a.gfx + ((long long)ycur * a.W + x) * a.ld + ch, v0, DRAG_FX_SCALE);
      if (ycur + 1 >= 0 && ycur + 1 < a.W) fx_add(a.gfx + ((long long)(ycur + 1) * a.W + x) * a.ld + ch, v1, DRAG_FX_SCALE);
    };
    // the segment's DSEG positions: all their texel loads are issued before the first is used.  Round 6: really -- written as
    // `if (in bounds) patch = fma(w, texel[...], patch)` every one of the 40 loads sat in a conditional block of its own, and the
    // compiler closes such a block with s_waitcnt vmcnt(0): 41 of the kernel's 46 waits stood right behind a load (26 us per step).
    // Now every load is unconditional at a clamped coordinate and a tap outside the map (zeros padding, drag_utils.py:355)
    // enters with value 0 and weight 0: fma(0, 0, acc) = acc, the same sums as skipping it, whatever the clamped texel holds.
    float dseg[DSEG];
    half_t tp[DSEG][4], te[DSEG][4];
    float wp[DSEG][4], we[DSEG][4];
#pragma unroll
    for (int ii = 0; ii < DSEG; ++ii) {
      const int i = seg * DSEG + ii;
      const Bilin bs = bilin_setup(lattice(su, a.voxel, i - a.r), sv, a.W);
      const Bilin bt = bilin_setup(lattice(tu, a.voxel, i - a.r), tv, a.W);
      const bool on = live && i < side;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int xs = bs.x0 + (q & 1), ys = bs.y0 + (q >> 1);
        const int xt = bt.x0 + (q & 1), yt = bt.y0 + (q >> 1);
        const int xsc = min(max(xs, 0), a.W - 1), ysc = min(max(ys, 0), a.W - 1);
        const int xtc = min(max(xt, 0), a.W - 1), ytc = min(max(yt, 0), a.W - 1);
        const half_t vp = a.orig[((long long)ysc * a.W + xsc) * a.ld + ch];
        const half_t ve = a.edit[((long long)ytc * a.W + xtc) * a.ld + ch];
        // the VALUE is selected as well as the weight (one v_cndmask behind the load, no extra wait): a clamped tap that reads a
        // non-finite border texel must not turn a sample outside the map into 0 * Inf = NaN; for finite texels the same bits
        const bool ins = on && xs == xsc && ys == ysc, ine = on && xt == xtc && yt == ytc;
        tp[ii][q] = ins ? vp : (half_t)0.f;
        te[ii][q] = ine ? ve : (half_t)0.f;
        wp[ii][q] = ins ? bs.w[q] : 0.f;
        we[ii][q] = ine ? bt.w[q] : 0.f;
      }
    }
#pragma unroll
    for (int ii = 0; ii < DSEG; ++ii) {
      float patch = 0.f, shift = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        // explicit fused multiply-adds on both sides: identical inputs must give shift == patch exactly
        patch = __fmaf_rn(wp[ii][q], (float)tp[ii][q], patch);
        shift = __fmaf_rn(we[ii][q], (float)te[ii][q], shift);
      }
      dseg[ii] = shift - patch;
    }
#pragma unroll
    for (int ii = 0; ii < DSEG; ++ii) {
      const int i = seg * DSEG + ii;
      if (i >= side) break;
      const Bilin bt = bilin_setup(lattice(tu, a.voxel, i - a.r), tv, a.W);
      const float d = dseg[ii];
      float g;
      if (a.l1) { if (live) lsum += mult * fabsf(d); g = -((d > 0.f) - (d < 0.f)) * mult / ntot; }
      else { if (live) lsum += mult * d * d; g = -2.f * d * mult / ntot; }
      if (!open || bt.x0 != xcur || bt.y0 != ycur) {         // wave-uniform: the coordinates do not depend on the lane
        if (open) {
          flush_col(xcur, a00, a10);
          if (bt.x0 == xcur + 1 && bt.y0 == ycur) { a00 = a01; a10 = a11; }
          else { flush_col(xcur + 1, a01, a11); a00 = 0.f; a10 = 0.f; }
          a01 = 0.f; a11 = 0.f;
        }
        xcur = bt.x0; ycur = bt.y0; open = true;
      }
      a00 += bt.w[0] * g; a01 += bt.w[1] * g; a10 += bt.w[2] * g; a11 += bt.w[3] * g;
    }
    if (open) { flush_col(xcur, a00, a10); flush_col(xcur + 1, a01, a11); }
  }
  block_loss_add(lsum, a.acc + 0);
}

// touched[p][row][col]: the marks of drag_touch_marks (drag.h, shared with csrc/retarget.hip) land in global memory.
// Byte-wide atomic OR via the 32-bit word.
__device__ __forceinline__ void drag_touch_one(const DragArgs& a, int p, int b, int st, int i, int j) {
  drag_touch_marks(a, p, b, st, i, j, [&](long long o, unsigned bit) {
    atomicOr(reinterpret_cast<unsigned*>(a.touched + (o & ~3ll)), bit << (8 * (o & 3)));
  });
}

__device__ __forceinline__ void drag_count_body(const DragArgs& a) {
  __shared__ int red[256];
  int cnt = 0;
  for (int i = threadIdx.x; i < 3 * a.W * a.W; i += 256) cnt += (a.touched[i] & 1) ? 0 : 1;
  red[threadIdx.x] = cnt;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
  if (threadIdx.x == 0) a.nmask[0] = red[0];
}

// chw[p][ch] = number of (plane p, c) pairs that resize_feat_align maps to tap channel ch (0 or 1; 2 where the nearest
// resize repeats a channel): lets the gather pass below add the mask term per tap element without a scatter
__global__ void drag_chan_weight_kernel(DragArgs a) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 3 * a.ld) return;
  const int p = idx / a.ld, ch = idx - p * a.ld;
  int cnt = 0;
  for (int c = 0; c < a.Cc; ++c) cnt += a.chmap[p * a.Cc + c] == ch ? 1 : 0;
  a.chw[idx] = (unsigned char)min(cnt, 255);
}

// loss from the two fixed-point sums; leaves them zero for the next call
__device__ __forceinline__ void drag_finish(const DragArgs& a) {
  const int side = 2 * a.r + 1;
  // one thread, once per edit: formed in double from the two integers and rounded to float once (a chain of six float
  // operations here cost about a unit in the last place: measured 1.75e-7 -> 1.17e-7 on a loss of 0.76)
  const double ntot = 3.0 * (double)a.Cc * (double)a.B * (double)side * (double)side * (double)side;
  double loss = -((double)a.acc[0] * (1.0 / (double)DRAG_ACC_SCALE)) / ntot;
  if (a.cof > 0.f)
    loss -= (double)a.cof * ((double)a.acc[1] * (1.0 / (double)DRAG_ACC_SCALE)) / ((double)a.Cc * (double)a.nmask[0]);
  a.loss[0] = (float)loss;
  a.acc[0] = 0;
  a.acc[1] = 0;
}

// Gather pass: fixed-point scatter buffer (motion term) -> the fp32 gradient the ABI returns, plus the MASK term
// (drag_utils.py:376-381: cof * mean over the untouched texels of |edit - orig|^2 or |.|), which is elementwise in the tap's
// own layout once the channel map is inverted (chw) -- it used to be a second 2-million-atomic scatter.  The buffer is
// left zero for the next call (no memset launch); with `absmax_bits` the pass also finds max|g| for the loss scale.
//
// WEIGHTED (region-constrained edits, csrc/regions.hip): `wmap` [3][W][W] floats, one weight per plane texel, scales the mask term of
// an UNTOUCHED texel (0 frees it, > 1 holds it harder); a touched texel's weight is never used.  The per-element weight becomes
// sum_p untouched_p ? wmap_p * chw_p[k] : 0 in float.  With a map of exact ones that sum is the same small integer the unweighted
// form converts from int, and every operation behind it has the same shape: the results are bitwise those of WEIGHTED = false,
// which is what keeps "each edit's loss is bitwise its solo loss" for a batch that mixes edits with and without regions.
// The unweighted instantiation is the code it was before the parameter existed.
template <bool WEIGHTED>
__device__ __forceinline__ void drag_gather_body(const DragArgs& a, int blk, int nblk, unsigned* __restrict__ absmax_bits,
                                                 const float* __restrict__ wmap) {
  typedef long long ll2 __attribute__((ext_vector_type(2)));
  typedef unsigned char uc8 __attribute__((ext_vector_type(8)));
  const long long n = (long long)a.W * a.W * a.ld;
  const int WW = a.W * a.W;
  const bool mask = a.cof > 0.f;
  const float denom = (float)a.Cc * (float)a.nmask[0];
  float m = 0.f, lsum = 0.f;
  // a thread takes 8 consecutive channels of one texel (ld % 8 == 0): 16-byte accesses on every stream
  for (long long i = ((long long)blk * blockDim.x + threadIdx.x) * 8; i < n; i += (long long)nblk * blockDim.x * 8) {
    float g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int tex = (int)(i / a.ld), ch = (int)(i - (long long)tex * a.ld);
    const unsigned char t0 = a.touched[tex], t1 = a.touched[WW + tex], t2 = a.touched[2 * WW + tex];
    // the mask term's operands, requested together with the footprint bytes (round 6: they used to be issued behind the footprint
    // test and, plane by plane, inside conditional blocks -- each closed by an s_waitcnt vmcnt(0))
    const half8 e8 = *reinterpret_cast<const half8*>(a.edit + i), o8 = *reinterpret_cast<const half8*>(a.orig + i);
    uc8 cw[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) cw[p] = *reinterpret_cast<const uc8*>(a.chw + p * a.ld + ch);
    // the texel's three region weights ride with the loads above, unconditionally (a load in a conditional block of its own is
    // closed by a full wait); an unweighted instantiation has no such loads
    float rw[3] = {1.f, 1.f, 1.f};
    if constexpr (WEIGHTED) { rw[0] = wmap[tex]; rw[1] = wmap[WW + tex]; rw[2] = wmap[2 * WW + tex]; }
    if ((t0 | t1 | t2) & 2) {                       // a target footprint covers this texel on some plane
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const ll2 v = *reinterpret_cast<const ll2*>(a.gfx + i + 2 * q);
        *reinterpret_cast<ll2*>(a.gfx + i + 2 * q) = (ll2){0, 0};
        g[2 * q] = (float)v[0] * (1.f / DRAG_FX_SCALE);
        g[2 * q + 1] = (float)v[1] * (1.f / DRAG_FX_SCALE);
      }
    }
    if (mask) {
      const unsigned char tp[3] = {t0, t1, t2};
      float wf[8];
      if constexpr (WEIGHTED) {
#pragma unroll
        for (int k = 0; k < 8; ++k) wf[k] = 0.f;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
          const float wp = (tp[p] & 1) ? 0.f : rw[p];       // a select, not a branch: touched -> weight ignored
#pragma unroll
          for (int k = 0; k < 8; ++k) wf[k] += wp * (float)cw[p][k];
        }
      } else {
        int w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int p = 0; p < 3; ++p)
          if (!(tp[p] & 1)) {
#pragma unroll
            for (int k = 0; k < 8; ++k) w[k] += cw[p][k];
          }
#pragma unroll
        for (int k = 0; k < 8; ++k) wf[k] = (float)w[k];
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float d = (float)e8[k] - (float)o8[k], wk = wf[k];
        if (a.l1) { lsum += wk * fabsf(d); g[k] += wk * (-a.cof * (float)((d > 0.f) - (d < 0.f)) / denom); }
        else { lsum += wk * d * d; g[k] += wk * (-a.cof * 2.f * d / denom); }
      }
    }
    *reinterpret_cast<f32x4*>(a.grad + i) = (f32x4){g[0], g[1], g[2], g[3]};
    *reinterpret_cast<f32x4*>(a.grad + i + 4) = (f32x4){g[4], g[5], g[6], g[7]};
#pragma unroll
    for (int k = 0; k < 8; ++k) m = fmaxf(m, fabsf(g[k]));
  }
  if (mask) block_loss_add(lsum, a.acc + 1);
  if (absmax_bits) {
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    __shared__ float red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(absmax_bits, __float_as_uint(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))));
  }
}

// ---- fp32 gradient -> scaled fp16 cotangent (power-of-two loss scale chosen from max|g|) ----
__global__ void absmax_kernel(const float* __restrict__ g, long long n, unsigned* __restrict__ out_bits) {
  float m = 0.f;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    m = fmaxf(m, fabsf(g[i]));
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(out_bits, __float_as_uint(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))));   // one per workgroup
}
__device__ __forceinline__ float pick_scale(float m);
__global__ void pick_scale_kernel(const unsigned* __restrict__ bits, float* __restrict__ scale2) {
  const float sc = pick_scale(__uint_as_float(bits[0]));
  scale2[0] = sc;
  scale2[1] = 1.f / sc;
}
__device__ __forceinline__ float pick_scale(float m) {
  float sc = 1.f;
  if (m > 0.f && isfinite(m)) sc = exp2f(floorf(log2f(256.f / m)));
  return fminf(fmaxf(sc, 0x1p-20f), 0x1p+99f);      // both clamps are powers of two, so the scale is one for every m
}
__global__ void scale_to_f16_kernel(const float* __restrict__ g, half_t* __restrict__ o, const float* __restrict__ scale2,
                                    long long n) {
  const float sc = scale2[0];
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    o[i] = (half_t)(g[i] * sc);
}
int grad_to_scaled_f16_launch(const float* g, half_t* o, unsigned* bits, float* scale2, long long n, hipStream_t s) {
  ISHAP_CHECK_HIP(hipMemsetAsync(bits, 0, sizeof(unsigned), s));
  int blocks = (int)std::min<long long>((n + 255) / 256, 1024);
  hipLaunchKernelGGL(absmax_kernel, dim3(std::min(blocks, 512)), dim3(256), 0, s, g, n, bits);
  hipLaunchKernelGGL(pick_scale_kernel, dim3(1), dim3(1), 0, s, bits, scale2);
  hipLaunchKernelGGL(scale_to_f16_kernel, dim3(blocks), dim3(256), 0, s, g, o, scale2, n);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

// ==== the launches: E edits per call; one edit is E = 1 ====
// Every pass is one launch whose grid is the concatenation of one grid per edit: workgroup blk of edit e runs the body above on
// edit e's slice (drag_edit_args) with that edit's own workgroup count as its grid stride, whatever E is and whichever edits
// stand beside it.  So each edit's float partial sums are formed in the same groups and order as alone, its fixed-point totals
// are the same integers, and its loss and fp32 gradient are BITWISE those of a call with that edit alone -- by construction:
// the call with one edit runs these same kernels -- three launches per guided step whatever E is.
//
// One loss scale for the batch.  The cotangent is g * 2^k in fp16 with k picked from max|g| over ALL edits (so k_batch <= k_solo
// of every edit).  Multiplying by a power of two is exact in fp32, and the fp16 cast of g * 2^k_batch equals the solo cotangent
// times 2^(k_batch - k_solo) bit for bit wherever it stays a normal fp16 number.  The UNet input-gradient backward is linear in
// its cotangent and removes the scale at its end (scale2[1]); a power-of-two rescaling of all its fp16 intermediates is exact as
// long as none leaves the fp16 range.  One scale per batch therefore needs no change to the backward: only an edit whose
// gradient is 2^10+ times smaller than the largest one of the batch loses low bits to fp16 subnormals.
// drag_edit_args (edit e's slice of a DragBatchArgs) is in drag.h

// one thread per (handle, plane, source / target, lattice i, j) over the packed handles of all edits.  Which thread takes which
// tuple is free: drag_touch_one reads the handles and does nothing but atomicOr marks into `touched`, and OR commutes, so the
// bitmap is the same for every assignment of tuples to threads (the single-edit kernel this one replaced ordered them plane-major)
__global__ void drag_batch_touch_kernel(DragBatchArgs b) {
  const int side = 2 * b.base.r + 1;
  const int per = 3 * 2 * side * side;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= per * b.hoff[b.E]) return;
  const int h = idx / per;
  int e = 0;
  while (e + 1 < b.E && h >= b.hoff[e + 1]) ++e;
  int rem = idx - h * per;
  const int j = rem % side; rem /= side;
  const int i = rem % side; rem /= side;
  const int st = rem % 2;
  const int p = rem / 2;
  drag_touch_one(drag_edit_args(b, e), p, h - b.hoff[e], st, i, j);
}
__global__ void drag_batch_count_kernel(DragBatchArgs b) { drag_count_body(drag_edit_args(b, blockIdx.x)); }

__global__ __launch_bounds__(256) void drag_batch_terms_kernel(DragBatchArgs b, unsigned* absmax_bits) {
  if (absmax_bits && blockIdx.x == 0 && threadIdx.x == 0) absmax_bits[0] = 0u;   // for the atomicMax of the pass that follows
  int e = 0;
  while (e + 1 < b.E && (int)blockIdx.x >= b.tblk[e + 1]) ++e;       // workgroup-uniform
  drag_motion_body(drag_edit_args(b, e), blockIdx.x - b.tblk[e], b.tblk[e + 1] - b.tblk[e]);
}
__global__ __launch_bounds__(256) void drag_batch_gather_kernel(DragBatchArgs b, int blocks_per_edit, unsigned* __restrict__ absmax_bits) {
  const int e = blockIdx.x / blocks_per_edit;
  drag_gather_body<false>(drag_edit_args(b, e), blockIdx.x - e * blocks_per_edit, blocks_per_edit, absmax_bits, nullptr);
}
// The weighted form, launched only when the batch carries weight maps: edit e reads weights + e * wstride.  The maps are the
// kernel's own trailing parameters and not fields of DragArgs / DragBatchArgs, so the kernel-argument layout of every other drag
// kernel -- and with it their code -- is what it was (README round 6: an argument-struct change once cost 3 % per edit).
__global__ __launch_bounds__(256) void drag_batch_gather_weighted_kernel(DragBatchArgs b, int blocks_per_edit,
                                                                         unsigned* __restrict__ absmax_bits,
                                                                         const float* __restrict__ weights, long long wstride) {
  const int e = blockIdx.x / blocks_per_edit;
  drag_gather_body<true>(drag_edit_args(b, e), blockIdx.x - e * blocks_per_edit, blocks_per_edit, absmax_bits, weights + e * wstride);
}
__global__ void drag_batch_finish_kernel(DragBatchArgs b) {
  for (int e = 0; e < b.E; ++e) drag_finish(drag_edit_args(b, e));
}
// fp32 gradient -> fp16 cotangent as scale_to_f16_kernel, with the scale picked by every thread from max|g| (published by thread
// 0) and the drag losses finished here: three launches fewer per guided step
__global__ void drag_batch_scale_kernel(const float* __restrict__ g, half_t* __restrict__ o, const unsigned* __restrict__ bits,
                                        float* __restrict__ scale2, DragBatchArgs b, long long n) {
  const float sc = pick_scale(__uint_as_float(bits[0]));
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    scale2[0] = sc;
    scale2[1] = 1.f / sc;
    for (int e = 0; e < b.E; ++e) drag_finish(drag_edit_args(b, e));
  }
  for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (long long)gridDim.x * blockDim.x * 4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(g + i);
    *reinterpret_cast<half4*>(o + i) = (half4){(half_t)(v[0] * sc), (half_t)(v[1] * sc), (half_t)(v[2] * sc), (half_t)(v[3] * sc)};
  }
}

// the shape requirements of every drag call (api.hip checks only the pointers and dimensions of its structs)
int drag_batch_check(const DragBatchArgs& a) {
  ISHAP_REQUIRE(a.E >= 1 && a.E <= DRAG_MAX_EDITS, "drag batch: E must be in 1..32");
  ISHAP_REQUIRE((3 * a.base.W * a.base.W) % 4 == 0 && a.base.ld % 8 == 0,
                "drag: 3*W*W must be a multiple of 4 and the tap channels of 8");
  ISHAP_REQUIRE(a.hoff[0] == 0, "drag batch: handle_offsets[0] must be 0");
  for (int e = 0; e < a.E; ++e) ISHAP_REQUIRE(a.hoff[e + 1] > a.hoff[e], "drag batch: every edit needs at least one handle");
  return 0;
}

// buffers as ishap.h describes them; zeroes the scratch that every loss call leaves zero again
int drag_batch_setup_launch(DragBatchArgs& a, hipStream_t s) {
  ISHAP_TRY(drag_batch_check(a));
  const DragArgs& d = a.base;
  const int side = 2 * d.r + 1;
  const long long n = (long long)d.W * d.W * d.ld;
  ISHAP_CHECK_HIP(hipMemsetAsync(d.touched, 0, (size_t)a.E * 3 * d.W * d.W, s));
  ISHAP_CHECK_HIP(hipMemsetAsync(d.gfx, 0, (size_t)a.E * n * sizeof(long long), s));
  ISHAP_CHECK_HIP(hipMemsetAsync(d.acc, 0, (size_t)a.E * 2 * sizeof(long long), s));
  const int total = 3 * 2 * side * side * a.hoff[a.E];
  hipLaunchKernelGGL(drag_batch_touch_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(drag_batch_count_kernel, dim3(a.E), dim3(256), 0, s, a);
  hipLaunchKernelGGL(drag_chan_weight_kernel, dim3(ceil_div(3 * d.ld, 256)), dim3(256), 0, s, d);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

static unsigned gather_blocks(long long n) {
  constexpr int cap = 512;
  return (unsigned)std::min<long long>((n / 8 + 255) / 256, cap);
}

// Losses + fp32 gradients of the E edits in three launches (motion scatter, gather + mask, finish); with `cot` the third launch
// also writes the scaled fp16 cotangent (drag_batch_scale_kernel) and `bits` / `scale2` must be given.  `weights` (device
// [E][3][W][W] floats, edit e at + e * wstride; nullptr: none) selects the weighted gather pass.  Requires
// drag_batch_setup_launch on these buffers first.
int drag_batch_loss_launch(DragBatchArgs& a, half_t* cot, unsigned* bits, float* scale2, const float* weights, long long wstride,
                           hipStream_t s) {
  ISHAP_TRY(drag_batch_check(a));
  ISHAP_REQUIRE(!weights || a.E == 1 || wstride == 0 || wstride >= 3ll * a.base.W * a.base.W,
                "drag: weights_stride must be 0 (one map for all edits) or at least 3*W*W");
  if (!cot) bits = nullptr;
  // every workgroup of the terms and gather passes ends with same-address atomics (loss sum, max|g|) that serialise at ~10 ns
  // each: few, fat workgroups (the loops are grid-stride).  Terms: a wave per DSEG positions of a lattice row, at most `cap`
  // workgroups per edit (swept in round 2; no result file was kept, and the library no longer reads the cap from the environment:
  // not repeatable as is)
  constexpr int cap = 1024;
  const int side = 2 * a.base.r + 1;
  a.tblk[0] = 0;
  for (int e = 0; e < a.E; ++e) {
    const int nrows = 3 * (a.hoff[e + 1] - a.hoff[e]) * side * ((a.base.Cc + 63) / 64) * ((side + DSEG - 1) / DSEG);
    a.tblk[e + 1] = a.tblk[e] + min(ceil_div(nrows * 64, 256), cap);
  }
  hipLaunchKernelGGL(drag_batch_terms_kernel, dim3(a.tblk[a.E]), dim3(256), 0, s, a, bits);
  const long long n = (long long)a.base.W * a.base.W * a.base.ld;
  const unsigned gb = gather_blocks(n);
  if (weights)
    hipLaunchKernelGGL(drag_batch_gather_weighted_kernel, dim3(gb * a.E), dim3(256), 0, s, a, (int)gb, bits, weights, wstride);
  else
    hipLaunchKernelGGL(drag_batch_gather_kernel, dim3(gb * a.E), dim3(256), 0, s, a, (int)gb, bits);
  if (cot) {
    const long long nt = n * a.E;
    hipLaunchKernelGGL(drag_batch_scale_kernel, dim3((unsigned)std::min<long long>((nt / 4 + 255) / 256, 1024)), dim3(256), 0, s,
                       (const float*)a.base.grad, cot, (const unsigned*)bits, scale2, a, nt);
  } else {
    hipLaunchKernelGGL(drag_batch_finish_kernel, dim3(1), dim3(1), 0, s, a);
  }
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}
