// Direct triplane fitting (reference: drag_utils.py:473-550, train_triplane_opt): per Adam step
//   loss = BCEWithLogits(decoder(coord), gt) + 0.3 * mse(decoder(r), decoder(r + 0.01 * randn)) + 0.001 * l2reg + 0.01 * tvreg
// (l2reg / tvreg: axisnetworks.py:564-575), gradient on the three planes only, the MLP frozen.
//
// triplane_fit_kernel: forward AND backward of the decoder (axisnetworks.py:526-562) for the data batch and the random pairs
// in one launch, every matrix product on the exact-fp32 matrix cores (v_mfma_f32_32x32x2_f32).  One wave owns a 32-point
// tile: lane & 31 = point, lane >> 5 = which of the two K slots of an MFMA step it feeds.  As in decode.hip the weights
// are the A operand and the activations the B operand, so a layer's accumulators ARE the next layer's operands
// (register r of lane-half h = neuron kmap(r, h) of its 32-block).  One fp32 copy of W1 and W2 sits in LDS; the forward
// reads rows (W[out][in], ds_read_b128 of 4 consecutive inputs), the backward's W^T products read the same arrays with the
// indices swapped (32 consecutive outputs per lane half, ds_read_b32).  What the backward needs stays in registers: the 64
// Fourier phases (sin / cos are recomputed) and the two ReLU masks as 64-bit words.  The last backward product (d features
// = _B . d phases) swaps the operands so that its accumulator is [point][channel]: register r then holds, across the 32
// lanes of a half, the 32 channels of ONE point -- each bilinear tap's gradient is one global_atomic_add_f32 instruction
// over two 128-byte texel rows (cdna_hip_programming.md, Guideline 12).
// A random pair (r, r + delta) is one work item: the same lane of two tiles in the same wave, so the pair's difference and
// its cotangents +-2 * 0.3 * d / N never leave registers.  Float atomics: not bitwise repeatable (as decode_bwd.hip).
//
// triplane_reg_partials_kernel + triplane_reg_adam_kernel: sum e^2, (D_H e)^2, (D_W e)^2 per plane in double in a fixed
// order (first launch: fixed per-block partials; second launch: every block re-sums the partials in the same order), then
// the regulariser gradients 0.001 e / |e| + 0.01 D^T (D e) / |D e| are added to dplanes and torch's Adam step
// (torch/optim/adam.py, single-tensor form) is applied into a second planes buffer; dplanes is left zeroed.
// Given the same dplanes these two launches are bitwise repeatable.
#include "decode.h"

#define FLD 132   // row stride (floats) of W1 / W2 in LDS: 528 B = 16 B mod 256 -> conflict-free ds_read_b128
#define BLD 68    // row stride (floats) of _B [32][64] in LDS: 272 B
#define FIT_WAVES 4

namespace {

// this lane's base pointers into the LDS images; every read below is base + a compile-time offset (< 64 KB), which the
// ds_read immediate absorbs (index arithmetic on the array start instead makes the compiler keep hundreds of addresses)
struct FitLds {
  const float *W1r, *W2r;   // row reads W[32qo + l31][k + 4h]
  const float *W1c, *W2c;   // column reads W[k + 4h][32qo + l31]
  const float *Bf, *Bb;     // _B[c + 4h][32q + l31] and _B[l31][k + 4h]
  const float *b1, *b2, *w3;   // + 4h
};

// what the backward of one 32-point tile keeps in registers between its forward and its backward (the phases are
// recomputed: 32 of the tile's 1088 MFMAs)
struct FitTile {
  unsigned long long m1, m2;     // ReLU masks: bit 16q + r = neuron 32q + kmap(r, h)
  float z;                       // logit of this lane's point
};

// point i of a tile: kind 0 = data (coords[idx[i]]), 1 = r, 2 = r + 0.01 * noise (drag_utils.py:533-534)
__device__ __forceinline__ void fit_point(const FitArgs& a, int kind, long long i, float& cx, float& cy, float& cz) {
  if (kind == 0) {
    const long long j = a.idx[i];
    cx = a.coords[j * 3]; cy = a.coords[j * 3 + 1]; cz = a.coords[j * 3 + 2];
    return;
  }
  cx = a.rcoords[i * 3]; cy = a.rcoords[i * 3 + 1]; cz = a.rcoords[i * 3 + 2];
  if (kind == 2) {      // rounded as the reference: randn * 1e-2, then the add
    cx = __fadd_rn(cx, __fmul_rn(a.rnoise[i * 3], 0.01f));
    cy = __fadd_rn(cy, __fmul_rn(a.rnoise[i * 3 + 1], 0.01f));
    cz = __fadd_rn(cz, __fmul_rn(a.rnoise[i * 3 + 2], 0.01f));
  }
}

// bilinear taps of plane p (xy, yz, xz; align_corners, zero padding: axisnetworks.py:537-551): texel index or -1, weight
__device__ __forceinline__ void fit_taps(int p, float cx, float cy, float cz, int S, int (&tex)[4], float (&w)[4]) {
  const float u = (p == 1) ? cy : cx;
  const float v = (p == 0) ? cy : cz;
  const float ix = ((u + 1.f) / 2.f) * (float)(S - 1);
  const float iy = ((v + 1.f) / 2.f) * (float)(S - 1);
  const float fx = floorf(ix), fy = floorf(iy);
  const int x0 = (int)fx, y0 = (int)fy;
  const float wx1 = ix - fx, wx0 = (fx + 1.f) - ix;
  const float wy1 = iy - fy, wy0 = (fy + 1.f) - iy;
#pragma unroll
  for (int q = 0; q < 4; ++q) {     // nw, ne, sw, se
    const int xx = x0 + (q & 1), yy = y0 + (q >> 1);
    w[q] = ((q & 1) ? wx1 : wx0) * ((q >> 1) ? wy1 : wy0);
    tex[q] = (xx >= 0 && xx < S && yy >= 0 && yy < S) ? (p * S + yy) * S + xx : -1;
  }
}

// features (three bilinear samples, summed) and phases y = f @ _B of this lane's point: y[q][r] = phase 32q + kmap(r, h)
__device__ __forceinline__ void fit_phases(const FitArgs& a, const FitLds& L, float cx, float cy, float cz, int l31, int h,
                                           f32x16 (&y)[2]) {
  // ---- features: this lane's 16 channels {8g+4h+e}, summed over the three planes ----
  f32x4 f[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) f[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    int tex[4];
    float w[4];
    fit_taps(p, cx, cy, cz, a.S, tex, w);
    f32x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (tex[q] >= 0) {
        const float* tp = a.planes + (long long)tex[q] * 32 + 4 * h;
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] += w[q] * *reinterpret_cast<const f32x4*>(tp + 8 * g);
      }
#pragma unroll
    for (int g = 0; g < 4; ++g) f[g] += acc[g];
  }
  // ---- phases y = f @ _B: A = _B^T rows (32q + i), K = channels ----
  // (the K order of this product and of the two layers below -- 32-blocks, within a block the pairs (8g + e, 8g + 4 + e) of one
  // K = 2 instruction -- is restated in tests/decoder_ref.py:_fit_order for the kink filter's error bound: change both together)
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

__device__ __forceinline__ void fit_forward(const FitArgs& a, const FitLds& L, float b3, float cx, float cy, float cz, int l31,
                                            int h, FitTile& t) {
  const float two_pi = 6.2831855f;      // float32(2*np.pi), axisnetworks.py:89
  f32x16 y[2];
  fit_phases(a, L, cx, cy, cz, l31, h, y);
  // ---- Fourier features: blocks 0,1 = sin, 2,3 = cos ----
  f32x16 x1[4];
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float s, c;
      sincos_cw(two_pi * y[q][r], s, c);
      x1[q][r] = s;
      x1[2 + q][r] = c;
    }
  // ---- layer 1 ----
  f32x16 x2[4];
  t.m1 = 0ull;
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
      if (v > 0.f) t.m1 |= 1ull << (16 * qo + r);
      x2[qo][r] = fmaxf(v, 0.f);
    }
  }
  // ---- layer 2 and the output layer ----
  float partial = 0.f;
  t.m2 = 0ull;
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
        t.m2 |= 1ull << (16 * qo + r);
        partial += L.w3[n] * v;
      }
    }
  }
  partial += __shfl_xor(partial, 32);
  t.z = partial + b3;
}

// dz: d loss / d logit of this lane's point (0 for padding lanes).  Scatters d loss / d planes with float atomics.
__device__ __forceinline__ void fit_backward(const FitArgs& a, const FitLds& L, const FitTile& t, float dz, int kind,
                                             long long tile0, long long n, float cx, float cy, float cz, int l31, int h) {
  const float two_pi = 6.2831855f;
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
          const float bv = ((t.m2 >> (16 * q + r)) & 1ull) ? w3v[e] * dz : 0.f;
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(L.W2c[(32 * q + kmap(r, 0)) * FLD + 32 * qo], bv, acc, 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
    for (int r = 0; r < 16; ++r) g1[qo][r] = ((t.m1 >> (16 * qo + r)) & 1ull) ? acc[r] : 0.f;
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
          dff[qo] = __builtin_amdgcn_mfma_f32_32x32x2f32(L.W1c[(32 * q + 8 * g + e) * FLD + 32 * qo],
                                                         g1[q][4 * g + e], dff[qo], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
  }
  // ---- d phases: 2 pi (d sin * cos - d cos * sin) ----
  f32x16 y[2], dy[2];
  fit_phases(a, L, cx, cy, cz, l31, h, y);
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float s, c;
      sincos_cw(two_pi * y[q][r], s, c);
      dy[q][r] = two_pi * (dff[q][r] * c - dff[2 + q][r] * s);
    }
  // ---- d features^T [point][channel] = dy^T _B^T: A = dy (point rows), B = _B rows (channel columns) ----
  f32x16 df;
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
  // ---- scatter: register r = channel l31 of point kmap(r, h); one instruction = two 128-byte texel rows ----
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const long long i = tile0 + kmap(r, h);
    if (i < n) {
      float px, py, pz;
      fit_point(a, kind, i, px, py, pz);
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        int tex[4];
        float w[4];
        fit_taps(p, px, py, pz, a.S, tex, w);
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (tex[q] >= 0) atomicAdd(a.dplanes + (long long)tex[q] * 32 + l31, w[q] * df[r]);
      }
    }
  }
}

}  // namespace

__global__ __launch_bounds__(64 * FIT_WAVES) void triplane_fit_kernel(FitArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* sW1 = lds;                       // [128][FLD] W1[out][in]
  float* sW2 = sW1 + 128 * FLD;
  float* sB = sW2 + 128 * FLD;            // [32][BLD]  _B[channel][phase]
  float* sb1 = sB + 32 * BLD;
  float* sb2 = sb1 + 128;
  float* sw3 = sb2 + 128;
  const int tid = threadIdx.x;
  for (int i = tid; i < 128 * 128; i += 64 * FIT_WAVES) {
    const int r = i >> 7, k = i & 127;
    sW1[r * FLD + k] = a.W1[i];
    sW2[r * FLD + k] = a.W2[i];
  }
  for (int i = tid; i < 32 * 64; i += 64 * FIT_WAVES) sB[(i >> 6) * BLD + (i & 63)] = a.B[i];
  if (tid < 128) { sb1[tid] = a.b1[tid]; sb2[tid] = a.b2[tid]; sw3[tid] = a.w3[tid]; }
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const FitLds L{sW1 + l31 * FLD + 4 * h, sW2 + l31 * FLD + 4 * h, sW1 + 4 * h * FLD + l31, sW2 + 4 * h * FLD + l31,
                 sB + 4 * h * BLD + l31, sB + l31 * BLD + 4 * h, sb1 + 4 * h, sb2 + 4 * h, sw3 + 4 * h};
  const float b3 = a.b3[0];
  const long long npair = (a.nrand + 31) / 32, ndata = (a.nbatch + 31) / 32;
  float bce_sum = 0.f, mse_sum = 0.f;
  // the pair items (two tiles each) first, so that the lighter data items fill the tail
  for (long long item = (long long)blockIdx.x * FIT_WAVES + wave; item < npair + ndata;
       item += (long long)gridDim.x * FIT_WAVES) {
    // one code instance of the forward and of the backward (not one per tile kind: the unrolled bodies are large), looped
    // over the item's tiles: data item = one tile (kind 0); pair item = r (kind 1) and r + delta (kind 2)
    const bool pair = item < npair;
    const long long n = pair ? a.nrand : a.nbatch;
    const long long tile0 = (pair ? item : item - npair) * 32, i = tile0 + l31;
    const bool valid = i < n;
    const long long ii = valid ? i : n - 1;
    const int ntiles = pair ? 2 : 1;
    FitTile ta, tb;
#pragma nounroll
    for (int k = 0; k < ntiles; ++k) {
      float cx, cy, cz;
      fit_point(a, pair ? 1 + k : 0, ii, cx, cy, cz);
      FitTile t;
      fit_forward(a, L, b3, cx, cy, cz, l31, h, t);
      if (k == 0) ta = t; else tb = t;
    }
    float dza, dzb = 0.f;
    if (pair) {
      const float d = ta.z - tb.z;
      if (valid && h == 0) mse_sum += d * d;
      dza = valid ? 2.f * a.pair_w * d / (float)a.nrand : 0.f;
      dzb = -dza;
    } else {
      const float gt = a.gt[a.idx[ii]];
      const float z = ta.z;
      if (valid && h == 0) bce_sum += fmaxf(z, 0.f) - z * gt + log1pf(expf(-fabsf(z)));
      const float sig = 1.f / (1.f + expf(-z));
      dza = valid ? (sig - gt) / (float)a.nbatch : 0.f;
    }
#pragma nounroll
    for (int k = 0; k < ntiles; ++k) {
      float cx, cy, cz;
      fit_point(a, pair ? 1 + k : 0, ii, cx, cy, cz);
      fit_backward(a, L, k == 0 ? ta : tb, k == 0 ? dza : dzb, pair ? 1 + k : 0, tile0, n, cx, cy, cz, l31, h);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    bce_sum += __shfl_xor(bce_sum, o);
    mse_sum += __shfl_xor(mse_sum, o);
  }
  if (lane == 0) {
    if (a.nbatch > 0) atomicAdd(a.loss_parts, bce_sum / (float)a.nbatch);
    if (a.nrand > 0) atomicAdd(a.loss_parts + 1, mse_sum / (float)a.nrand);
  }
}

int triplane_fit_loss_grad_launch(const FitArgs& a, hipStream_t s) {
  ISHAP_REQUIRE(a.nbatch >= 0 && a.nrand >= 0 && a.nbatch + a.nrand > 0, "no points");
  ISHAP_REQUIRE(a.S >= 2, "triplane fit_loss_grad: plane size");
  const size_t smem = (size_t)(2 * 128 * FLD + 32 * BLD + 3 * 128) * sizeof(float);
  ISHAP_TRY(ishap_set_max_lds((const void*)triplane_fit_kernel, (int)smem));
  const long long items = (a.nrand + 31) / 32 + (a.nbatch + 31) / 32;
  const int blocks = (int)std::min<long long>((items + FIT_WAVES - 1) / FIT_WAVES, 256);
  hipLaunchKernelGGL(triplane_fit_kernel, dim3(blocks), dim3(64 * FIT_WAVES), smem, s, a);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ regularisers and Adam
// ws[(p * TRIPLANE_REG_BLOCKS + b) * 3 + {0,1,2}] = block b's share of sum e^2, sum (D_H e)^2, sum (D_W e)^2 of plane p.
// D_H e = e[y+1][x] - e[y][x] (the reference's embed[:, :, 1:] - embed[:, :, :-1]), D_W along x; planes [p][y][x][c].
__global__ __launch_bounds__(256) void triplane_reg_partials_kernel(const float* __restrict__ planes, int S, double* ws,
                                                                    int* step) {
  __shared__ double red[3][256];
  const int p = blockIdx.y, b = blockIdx.x, tid = threadIdx.x;
  const long long n = (long long)S * S * 32;
  const long long chunk = (n + TRIPLANE_REG_BLOCKS - 1) / TRIPLANE_REG_BLOCKS;
  const long long i0 = b * chunk, i1 = std::min(n, i0 + chunk);
  const float* pl = planes + p * n;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (long long i = i0 + tid; i < i1; i += 256) {
    const float e = pl[i];
    const long long pix = i >> 5;
    const int x = (int)(pix % S), y = (int)(pix / S);
    s0 += (double)e * e;
    if (y + 1 < S) { const float d = pl[i + 32 * S] - e; s1 += (double)d * d; }
    if (x + 1 < S) { const float d = pl[i + 32] - e; s2 += (double)d * d; }
  }
  red[0][tid] = s0; red[1][tid] = s1; red[2][tid] = s2;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o)
      for (int k = 0; k < 3; ++k) red[k][tid] += red[k][tid + o];
    __syncthreads();
  }
  if (tid < 3) ws[(p * TRIPLANE_REG_BLOCKS + b) * 3 + tid] = red[tid][0];
  if (step && p == 0 && b == 0 && tid == 0) *step += 1;
}

__global__ __launch_bounds__(256) void triplane_reg_adam_kernel(RegAdamArgs a) {
  __shared__ double nrm[3][3];
  const int tid = threadIdx.x;
  if (tid < 9) {          // fixed order: every block gets the same bits
    const int p = tid / 3, k = tid % 3;
    double s = 0.0;
    for (int b = 0; b < TRIPLANE_REG_BLOCKS; ++b) s += a.ws[(p * TRIPLANE_REG_BLOCKS + b) * 3 + k];
    nrm[p][k] = sqrt(s);
  }
  __syncthreads();
  if (blockIdx.x == 0 && tid == 0 && a.reg_parts) {
    a.reg_parts[0] = (float)((nrm[0][0] + nrm[1][0]) + nrm[2][0]);
    a.reg_parts[1] = (float)(((nrm[0][1] + nrm[0][2]) + (nrm[1][1] + nrm[1][2])) + (nrm[2][1] + nrm[2][2]));
  }
  if (!a.planes_out) return;
  const int S = a.S;
  const long long n = (long long)S * S * 32;
  const int t = *a.step;
  const double bc1 = 1.0 - pow(a.beta1, (double)t), bc2 = 1.0 - pow(a.beta2, (double)t);
  const float step_size = (float)(a.lr / bc1), bc2_sqrt = (float)sqrt(bc2);
  const float omb1 = (float)(1.0 - a.beta1), b2 = (float)a.beta2, omb2 = (float)(1.0 - a.beta2), eps = (float)a.eps;
  for (long long i = (long long)blockIdx.x * blockDim.x + tid; i < 3 * n; i += (long long)gridDim.x * blockDim.x) {
    const int p = (int)(i / n);
    const long long j = i - p * n, pix = j >> 5;
    const int x = (int)(pix % S), y = (int)(pix / S);
    const float* pl = a.planes + p * n;
    const float e = pl[j];
    // D^T (D e) at this element: (e - e[prev]) - (e[next] - e), each term where it exists
    float gh = 0.f, gw = 0.f;
    if (y > 0) gh += e - pl[j - 32 * S];
    if (y + 1 < S) gh -= pl[j + 32 * S] - e;
    if (x > 0) gw += e - pl[j - 32];
    if (x + 1 < S) gw -= pl[j + 32] - e;
    const float i0 = nrm[p][0] > 0.0 ? (float)(1.0 / nrm[p][0]) : 0.f;
    const float i1 = nrm[p][1] > 0.0 ? (float)(1.0 / nrm[p][1]) : 0.f;
    const float i2 = nrm[p][2] > 0.0 ? (float)(1.0 / nrm[p][2]) : 0.f;
    const float g = a.dplanes[i] + a.l2_w * (e * i0) + a.tv_w * (gh * i1 + gw * i2);
    float m = a.m[i], v = a.v[i];
    m = m + omb1 * (g - m);                 // exp_avg.lerp_(grad, 1 - beta1)
    v = v * b2 + omb2 * (g * g);            // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    a.m[i] = m;
    a.v[i] = v;
    a.planes_out[i] = e - step_size * (m / denom);
    a.dplanes[i] = 0.f;
  }
}

int triplane_reg_adam_launch(const RegAdamArgs& a, hipStream_t s) {
  ISHAP_REQUIRE(a.S >= 2 && a.planes && a.ws, "null argument");
  const bool adam = a.planes_out != nullptr;
  ISHAP_REQUIRE(!adam || (a.m && a.v && a.dplanes && a.step), "null Adam state");
  ISHAP_REQUIRE(adam || a.reg_parts, "nothing to write");
  ISHAP_REQUIRE(a.planes_out != a.planes, "planes_out must not alias planes");
  hipLaunchKernelGGL(triplane_reg_partials_kernel, dim3(TRIPLANE_REG_BLOCKS, 3), dim3(256), 0, s, a.planes, a.S, a.ws,
                     adam ? a.step : nullptr);
  ISHAP_CHECK_HIP(hipGetLastError());
  const long long total = 3LL * a.S * a.S * 32;
  const int blocks = adam ? (int)std::min<long long>((total + 255) / 256, 1024) : 1;
  hipLaunchKernelGGL(triplane_reg_adam_kernel, dim3(blocks), dim3(256), 0, s, a);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}
