// The triplane decoder's MLP (MultiTriplane.forward, axisnetworks.py:526-562) for one 32-point tile per wave, every matrix
// product on the exact-fp32 matrix cores (v_mfma_f32_32x32x2_f32): the ONE statement of the tile scheme that
// triplane_fit_kernel (decode_fit.hip) and triplane_field_kernel / triplane_project_kernel (decode_field.hip) are built on.
//
// One wave owns 32 points: lane & 31 = point, lane >> 5 = which of the two K slots of an MFMA step the lane feeds.  As in
// decode.hip the weights are the A operand and the activations the B operand, so a layer's accumulators ARE the next
// layer's operands (register r of lane-half h = neuron kmap(r, h) of its 32-block).  One fp32 copy of W1, W2 and _B sits in
// LDS; the forward reads rows (W[out][in], ds_read_b128 of 4 consecutive inputs), the backward's W^T products read the same
// arrays with the indices swapped (32 consecutive outputs per lane half, ds_read_b32).  Between forward and backward a
// caller keeps the two ReLU masks as 64-bit words; the 64 Fourier phases are recomputed (32 of a tile's 1088 MFMAs).  The
// last backward product (d features = _B . d phases) swaps its operands so that the accumulator is [point][channel]:
// register r of lane (l31, h) = channel l31 of point kmap(r, h).
//
// The K order of the products -- 32-blocks, within a block the pairs (8g + e, 8g + 4 + e) of one K = 2 instruction, bias
// last -- is restated in tests/decoder_ref.py:_fit_order for the kink filter's error bound: change both together.
//
// Rounding.  Every function below that does float arithmetic opens with `#pragma clang fp contract(off)` (at file scope
// it would stay in force for the rest of the including file, and decode_fit.hip's own code is compiled with the default
// contraction), so a mul and an add here are what the source says, whatever mode the including file is compiled in.  The two kernel families differ on
// purpose at two sites, the bilinear tap accumulation (mlp_muladd<FUSED>) and d phases (mlp_mulsub<FUSED>): the fit
// (FUSED = true) rounds once, a fused multiply-add, as the compiler's default contraction had made it; the field kernels
// (FUSED = false) round the product and the sum separately, so that the two of them, which inline the same evaluation,
// cannot come to differ by a fusion.  The w3 sum of the output layer is a fused multiply-add for every caller.
#pragma once
#include "decode.h"

#define FLD 132   // row stride (floats) of W1 / W2 in LDS: 528 B = 16 B mod 256 -> conflict-free ds_read_b128
#define BLD 68    // row stride (floats) of _B [32][64] in LDS: 272 B
#define MLP_SMEM ((size_t)(2 * 128 * FLD + 32 * BLD + 3 * 128) * sizeof(float))     // dynamic shared memory of a kernel

// this lane's base pointers into the LDS images; every read below is base + a compile-time offset (< 64 KB), which the
// ds_read immediate absorbs (index arithmetic on the array start instead makes the compiler keep hundreds of addresses)
struct MlpLds {
  const float *W1r, *W2r;   // row reads W[32qo + l31][k + 4h]
  const float *W1c, *W2c;   // column reads W[k + 4h][32qo + l31]
  const float *Bf, *Bb;     // _B[c + 4h][32q + l31] and _B[l31][k + 4h]
  const float *b1, *b2, *w3;   // + 4h
};

// fills the LDS images from a's weights (FitArgs / FieldArgs) with all THREADS threads of the workgroup, ends in the
// __syncthreads(), and returns this lane's pointers
template <int THREADS, class Args>
__device__ __forceinline__ MlpLds mlp_fill_lds(const Args& a, float* lds, int tid) {
  float* sW1 = lds;                       // [128][FLD] W1[out][in]
  float* sW2 = sW1 + 128 * FLD;
  float* sB = sW2 + 128 * FLD;            // [32][BLD]  _B[channel][phase]
  float* sb1 = sB + 32 * BLD;
  float* sb2 = sb1 + 128;
  float* sw3 = sb2 + 128;
  for (int i = tid; i < 128 * 128; i += THREADS) {
    const int r = i >> 7, k = i & 127;
    sW1[r * FLD + k] = a.W1[i];
    sW2[r * FLD + k] = a.W2[i];
  }
  for (int i = tid; i < 32 * 64; i += THREADS) sB[(i >> 6) * BLD + (i & 63)] = a.B[i];
  if (tid < 128) { sb1[tid] = a.b1[tid]; sb2[tid] = a.b2[tid]; sw3[tid] = a.w3[tid]; }
  __syncthreads();
  const int l31 = tid & 31, h = (tid >> 5) & 1;
  return MlpLds{sW1 + l31 * FLD + 4 * h, sW2 + l31 * FLD + 4 * h, sW1 + 4 * h * FLD + l31, sW2 + 4 * h * FLD + l31,
                sB + 4 * h * BLD + l31, sB + l31 * BLD + 4 * h, sb1 + 4 * h, sb2 + 4 * h, sw3 + 4 * h};
}

// a * b + c with one rounding (FUSED) or two
template <bool FUSED>
__device__ __forceinline__ f32x4 mlp_muladd(float a, f32x4 b, f32x4 c) {
#pragma clang fp contract(off)
  return FUSED ? __builtin_elementwise_fma((f32x4){a, a, a, a}, b, c) : a * b + c;
}

// a * b - c * d: FUSED rounds c * d, then fma(a, b, -cd) (of the two ways to contract it, the one the compiler took)
template <bool FUSED>
__device__ __forceinline__ float mlp_mulsub(float a, float b, float c, float d) {
#pragma clang fp contract(off)
  return FUSED ? fmaf(a, b, -(c * d)) : a * b - c * d;
}

// bilinear cell of plane p (xy, yz, xz; align_corners, zero padding: axisnetworks.py:537-551): the four texel indices
// (nw ne sw se, -1 = out of range) and the axis weights; tap q weighs wx[q & 1] * wy[q >> 1]
__device__ __forceinline__ void mlp_cell(int p, float cx, float cy, float cz, int S, int (&tex)[4], float (&wx)[2],
                                         float (&wy)[2]) {
#pragma clang fp contract(off)
  const float u = (p == 1) ? cy : cx;
  const float v = (p == 0) ? cy : cz;
  const float ix = ((u + 1.f) / 2.f) * (float)(S - 1);
  const float iy = ((v + 1.f) / 2.f) * (float)(S - 1);
  const float fx = floorf(ix), fy = floorf(iy);
  // a coordinate beyond +-2^30 texels has no tap in range either way: keep the conversion defined
  const int x0 = (int)fminf(fmaxf(fx, -2.f), 1073741824.f), y0 = (int)fminf(fmaxf(fy, -2.f), 1073741824.f);
  wx[1] = ix - fx; wx[0] = (fx + 1.f) - ix;
  wy[1] = iy - fy; wy[0] = (fy + 1.f) - iy;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int xx = x0 + (q & 1), yy = y0 + (q >> 1);
    tex[q] = (xx >= 0 && xx < S && yy >= 0 && yy < S) ? (p * S + yy) * S + xx : -1;
  }
}

// features (three bilinear samples, summed) and phases y = f @ _B of this lane's point: y[q][r] = phase 32q + kmap(r, h)
template <bool FUSED>
__device__ __forceinline__ void mlp_phases(const float* __restrict__ planes, int S, const MlpLds& L, float cx, float cy,
                                           float cz, int h, f32x16 (&y)[2]) {
#pragma clang fp contract(off)
  f32x4 f[4];       // this lane's 16 channels {8g + 4h + e}
#pragma unroll
  for (int g = 0; g < 4; ++g) f[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    int tex[4];
    float wx[2], wy[2];
    mlp_cell(p, cx, cy, cz, S, tex, wx, wy);
    f32x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (tex[q] >= 0) {
        const float w = wx[q & 1] * wy[q >> 1];
        const float* tp = planes + (long long)tex[q] * 32 + 4 * h;
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = mlp_muladd<FUSED>(w, *reinterpret_cast<const f32x4*>(tp + 8 * g), acc[g]);
      }
#pragma unroll
    for (int g = 0; g < 4; ++g) f[g] += acc[g];
  }
  // ---- y = f @ _B: A = _B^T rows (32q + i), K = channels ----
#pragma unroll
  for (int q = 0; q < 2; ++q) {
#pragma unroll
    for (int r = 0; r < 16; ++r) y[q][r] = 0.f;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        y[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(L.Bf[(8 * g + e) * BLD + 32 * q], f[g][e], y[q], 0, 0, 0);
  }
}

#define MLP_TWO_PI 6.2831855f      // float32(2*np.pi), axisnetworks.py:89

// forward of this lane's point (cx, cy, cz): the logit z (the same bits in both lane halves) and the ReLU masks of the two
// hidden layers, bit 16q + r = neuron 32q + kmap(r, h).  Wave-collective: all 64 lanes must call it.
template <bool FUSED>
__device__ __forceinline__ void mlp_forward(const float* __restrict__ planes, int S, const MlpLds& L, float b3, float cx,
                                            float cy, float cz, int h, unsigned long long& m1, unsigned long long& m2,
                                            float& z) {
#pragma clang fp contract(off)
  f32x16 y[2];
  mlp_phases<FUSED>(planes, S, L, cx, cy, cz, h, y);
  f32x16 x1[4];       // Fourier features: blocks 0,1 = sin, 2,3 = cos
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float s, c;
      sincos_cw(MLP_TWO_PI * y[q][r], s, c);
      x1[q][r] = s;
      x1[2 + q][r] = c;
    }
  // ---- layer 1 ----
  f32x16 x2[4];
  m1 = 0ull;
#pragma unroll
  for (int qo = 0; qo < 4; ++qo) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(L.W1r + 32 * qo * FLD + 32 * q + 8 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[e], x1[q][4 * g + e], acc, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);      // keep the weight reads next to their MFMAs (hoisted, they spill)
      }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float v = acc[r] + L.b1[32 * qo + kmap(r, 0)];
      if (v > 0.f) m1 |= 1ull << (16 * qo + r);
      x2[qo][r] = fmaxf(v, 0.f);
    }
  }
  // ---- layer 2 and the output layer ----
  float partial = 0.f;
  m2 = 0ull;
#pragma unroll
  for (int qo = 0; qo < 4; ++qo) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 wv = *reinterpret_cast<const f32x4*>(L.W2r + 32 * qo * FLD + 32 * q + 8 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[e], x2[q][4 * g + e], acc, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = 32 * qo + kmap(r, 0);
      const float v = acc[r] + L.b2[n];
      if (v > 0.f) {
        m2 |= 1ull << (16 * qo + r);
        partial = fmaf(L.w3[n], v, partial);
      }
    }
  }
  z = (partial + __shfl_xor(partial, 32)) + b3;
}

// backward of the same point from dz = d loss / d logit (0 for a padding lane; the literal 1.f for the field itself) to
// the feature cotangent df [point][channel]: df[r] of lane (l31, h) = channel l31 of point kmap(r, h).  Wave-collective.
template <bool FUSED>
__device__ __forceinline__ void mlp_backward(const float* __restrict__ planes, int S, const MlpLds& L,
                                             unsigned long long m1, unsigned long long m2, float dz, float cx, float cy,
                                             float cz, int h, f32x16& df) {
#pragma clang fp contract(off)
  // ---- d h1 = W2^T (w3 * dz * relu'(h2)), masked by relu'(h1) ----
  f32x16 g1[4];
#pragma unroll
  for (int qo = 0; qo < 4; ++qo) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 w3v = *reinterpret_cast<const f32x4*>(L.w3 + 32 * q + 8 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * g + e;
          const float bv = ((m2 >> (16 * q + r)) & 1ull) ? w3v[e] * dz : 0.f;
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(L.W2c[(32 * q + kmap(r, 0)) * FLD + 32 * qo], bv, acc, 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
    for (int r = 0; r < 16; ++r) g1[qo][r] = ((m1 >> (16 * qo + r)) & 1ull) ? acc[r] : 0.f;
  }
  // ---- d Fourier features = W1^T g1 ----
  f32x16 dff[4];
#pragma unroll
  for (int qo = 0; qo < 4; ++qo) {
#pragma unroll
    for (int r = 0; r < 16; ++r) dff[qo][r] = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          dff[qo] = __builtin_amdgcn_mfma_f32_32x32x2f32(L.W1c[(32 * q + 8 * g + e) * FLD + 32 * qo], g1[q][4 * g + e],
                                                         dff[qo], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
  }
  // ---- d phases: 2 pi (d sin * cos - d cos * sin), the phases recomputed ----
  f32x16 y[2], dy[2];
  mlp_phases<FUSED>(planes, S, L, cx, cy, cz, h, y);
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float s, c;
      sincos_cw(MLP_TWO_PI * y[q][r], s, c);
      dy[q][r] = MLP_TWO_PI * mlp_mulsub<FUSED>(dff[q][r], c, dff[2 + q][r], s);
    }
  // ---- d features^T [point][channel] = dy^T _B^T: A = dy (point rows), B = _B rows (channel columns) ----
#pragma unroll
  for (int r = 0; r < 16; ++r) df[r] = 0.f;
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 bv = *reinterpret_cast<const f32x4*>(L.Bb + 32 * q + 8 * g);
#pragma unroll
      for (int e = 0; e < 4; ++e) df = __builtin_amdgcn_mfma_f32_32x32x2f32(dy[q][4 * g + e], bv[e], df, 0, 0, 0);
    }
}
