// Volume constraints of a drag edit: L = -(1 / Wsum) sum_j w_j BCEWithLogits(decoder(planes)(q_j), g_j) at fixed points q_j
// and d L / d planes, bitwise repeatable (the sign convention of the reference's drag_utils.py:457; extends
// decode_points_bwd_kernel of decode_bwd.hip, which scatters with float atomics and has no weights).
//
// constraint_setup_launch, once per edit.  The 12 bilinear taps of every point (three planes x the four taps of mlp_cell)
// are grouped by the texel row they touch: integer atomics count the taps of each row, scan_exclusive_u32 turns the counts
// into row_start, a fill drops (4 j + q, weight) into its row in whatever order the integer atomics hand out, and a ranking
// pass (one wave per row: an entry's place is the number of smaller keys in its row; the keys of a row are distinct, because
// the row fixes the plane) writes them in ascending order.  The three outputs depend on the coordinates alone.  The ranking
// costs (entries of a row)^2 / 64 steps per row: points of a voxel grid put a few hundred entries into a row at the most.
//
// constraint_loss_grad_launch, once per step, two launches.
//   constraint_point_kernel: the tile scheme of decode_mlp.h as triplane_field_kernel runs it -- one wave per 32 points,
//     mlp_forward<false>, dz = -w (sigmoid(z) - g) / Wsum, mlp_backward<false> -- and the feature cotangent of every point
//     stored as one row dfeat[j][32] (the three planes share it: the features are their sum).  A tile's sum of w * bce, by a
//     fixed xor butterfly, goes to partials[tile].  A padding lane evaluates a stand-in point with dz = 0 and stores nothing.
//   constraint_gather_kernel: lane = channel, 32 lanes per texel row: dplanes[row][c] = sum over the row's entries, in entry
//     order, of entry_w * dfeat[j][c], product and sum rounded separately; a row without entries is written as 0.0, so the
//     buffer needs no memset.  One thread adds the tile partials in tile order in double and writes the loss.
#include "constrain.h"
#include "decode_mlp.h"
#include "scan.h"

#pragma clang fp contract(off)

#define CONSTRAINT_WAVES 4
#define CONSTRAINT_MAX_BLOCKS 256
#define CONSTRAINT_GATHER_ROWS 8      // texel rows per workgroup of the gather pass (32 lanes each)

namespace {

// tap t = 4 p + q of point j: its texel row (-1: out of range) and weight
__device__ __forceinline__ int tap_row(const float* __restrict__ coords, long long j, int t, int S, float& w) {
  const int p = t >> 2, q = t & 3;
  int tex[4];
  float wx[2], wy[2];
  mlp_cell(p, coords[j * 3], coords[j * 3 + 1], coords[j * 3 + 2], S, tex, wx, wy);
  w = wx[q & 1] * wy[q >> 1];
  return tex[q];
}

__global__ __launch_bounds__(256) void constraint_count_kernel(const float* __restrict__ coords, long long M, int S,
                                                               unsigned* __restrict__ count) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < 12 * M; i += (long long)gridDim.x * blockDim.x) {
    float w;
    const int row = tap_row(coords, i / 12, (int)(i % 12), S, w);
    if (row >= 0) atomicAdd(count + row, 1u);
  }
}

__global__ __launch_bounds__(256) void constraint_cursor_kernel(const unsigned* __restrict__ row_start, long long rows,
                                                                unsigned* __restrict__ cursor) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < rows; i += (long long)gridDim.x * blockDim.x)
    cursor[i] = row_start[i];
}

__global__ __launch_bounds__(256) void constraint_fill_kernel(const float* __restrict__ coords, long long M, int S,
                                                              unsigned* __restrict__ cursor, int* __restrict__ key,
                                                              float* __restrict__ keyw) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < 12 * M; i += (long long)gridDim.x * blockDim.x) {
    float w;
    const long long j = i / 12;
    const int t = (int)(i % 12);
    const int row = tap_row(coords, j, t, S, w);
    if (row >= 0) {
      const unsigned pos = atomicAdd(cursor + row, 1u);     // < row_start[row + 1]: the count pass saw the same taps
      key[pos] = (int)(4 * j + (t & 3));
      keyw[pos] = w;
    }
  }
}

// one wave per row: entry i goes to the place (number of smaller keys of its row)
__global__ __launch_bounds__(256) void constraint_rank_kernel(const int* __restrict__ row_start, long long rows,
                                                              const int* __restrict__ key, const float* __restrict__ keyw,
                                                              int* __restrict__ entry, float* __restrict__ entry_w) {
  const int lane = threadIdx.x & 63;
  for (long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (long long)gridDim.x * 4) {
    const int b = row_start[row], n = row_start[row + 1] - b;
    for (int i = lane; i < n; i += 64) {
      const int k = key[b + i];
      int rank = 0;
      for (int o = 0; o < n; ++o) rank += key[b + o] < k;
      entry[b + rank] = k;
      entry_w[b + rank] = keyw[b + i];
    }
  }
}

__global__ __launch_bounds__(64 * CONSTRAINT_WAVES) void constraint_point_kernel(ConstraintArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x;
  const MlpLds L = mlp_fill_lds<64 * CONSTRAINT_WAVES>(a, lds, tid);
  const int lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const float b3 = a.b3[0];
  const long long ntiles = (a.npts + 31) / 32;
  for (long long tile = (long long)blockIdx.x * CONSTRAINT_WAVES + wave; tile < ntiles;
       tile += (long long)gridDim.x * CONSTRAINT_WAVES) {
    const long long i = tile * 32 + l31;
    const bool valid = i < a.npts;
    const long long ii = valid ? i : a.npts - 1;
    const float cx = a.coords[ii * 3], cy = a.coords[ii * 3 + 1], cz = a.coords[ii * 3 + 2];
    const float gt = a.gt[ii], pw = valid ? a.pw[ii] : 0.f;
    unsigned long long m1, m2;
    float z;
    mlp_forward<false>(a.planes, a.S, L, b3, cx, cy, cz, h, m1, m2, z);
    // BCE-with-logits and d L / dz in the saturation-safe forms of decode_points_bwd_kernel
    const float sig = 1.f / (1.f + expf(-z));
    const float dz = valid ? -(pw * (sig - gt)) / a.wsum : 0.f;
    float part = 0.f;
    if (valid && h == 0) {
      part = pw * (fmaxf(z, 0.f) - z * gt + log1pf(expf(-fabsf(z))));
      if (a.logits) a.logits[i] = z;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
    if (lane == 0) a.partials[tile] = part;
    f32x16 df;
    mlp_backward<false>(a.planes, a.S, L, m1, m2, dz, cx, cy, cz, h, df);
    // register r of lane (l31, h) = channel l31 of point kmap(r, h): 32 lanes store one 128-byte row
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long long pt = tile * 32 + kmap(r, h);
      if (pt < a.npts) a.dfeat[pt * 32 + l31] = df[r];
    }
  }
}

__global__ __launch_bounds__(32 * CONSTRAINT_GATHER_ROWS) void constraint_gather_kernel(ConstraintArgs a, long long rows,
                                                                                        long long ntiles) {
  const int c = threadIdx.x & 31;
  const long long row = (long long)blockIdx.x * CONSTRAINT_GATHER_ROWS + (threadIdx.x >> 5);
  if (row < rows) {
    const int b = a.row_start[row], e = a.row_start[row + 1];
    float acc = 0.f;
    for (int k = b; k < e; ++k) {
      const float prod = a.entry_w[k] * a.dfeat[(long long)(a.entry[k] >> 2) * 32 + c];
      acc = acc + prod;
    }
    a.dplanes[row * 32 + c] = acc;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double sum = 0.0;
    for (long long t = 0; t < ntiles; ++t) sum += (double)a.partials[t];
    a.loss[0] = (float)(-sum / (double)a.wsum);
  }
}

struct SetupScratch {
  unsigned *totals, *cursor;
  int* key;
  float* keyw;
  size_t bytes;
};

SetupScratch setup_scratch(void* base, long long M, int S) {
  const size_t rows = (size_t)3 * S * S;
  Carve c{(char*)base};
  return {c.take<unsigned>(scan_u32_blocks((long long)rows + 1) + 1), c.take<unsigned>(rows), c.take<int>((size_t)12 * M),
          c.take<float>((size_t)12 * M), (size_t)c.total()};
}

bool sizes_ok(long long M, int S) { return M >= 1 && M <= CONSTRAINT_MAX_POINTS && S >= 2 && S <= CONSTRAINT_MAX_S; }

}  // namespace

long long constraint_setup_scratch_bytes(long long M, int S) {
  if (!sizes_ok(M, S)) return -1;
  return (long long)setup_scratch(nullptr, M, S).bytes;
}

int constraint_setup_launch(const ConstraintSetupArgs& a, hipStream_t s) {
  ISHAP_REQUIRE(sizes_ok(a.M, a.S), "constraint setup: 1 <= M <= 2^20 points and 2 <= S <= 1024");
  ISHAP_REQUIRE(a.coords && a.row_start && a.entry && a.entry_w && a.scratch, "null argument");
  const SetupScratch sc = setup_scratch(a.scratch, a.M, a.S);
  ISHAP_REQUIRE(a.scratch_bytes >= (long long)sc.bytes, "constraint setup: scratch too small (ishap_constraint_setup_scratch_bytes)");
  const long long rows = (long long)3 * a.S * a.S, taps = 12 * a.M;
  unsigned* count = (unsigned*)a.row_start;
  ISHAP_CHECK_HIP(hipMemsetAsync(count, 0, (size_t)(rows + 1) * sizeof(unsigned), s));
  const int tap_blocks = (int)std::min<long long>((taps + 255) / 256, 4096);
  hipLaunchKernelGGL(constraint_count_kernel, dim3(tap_blocks), dim3(256), 0, s, a.coords, a.M, a.S, count);
  scan_exclusive_u32(count, rows + 1, sc.totals, nullptr, s);      // count[rows] = 0: row_start[rows] = the entry count
  hipLaunchKernelGGL(constraint_cursor_kernel, dim3((int)std::min<long long>((rows + 255) / 256, 4096)), dim3(256), 0, s, count,
                     rows, sc.cursor);
  hipLaunchKernelGGL(constraint_fill_kernel, dim3(tap_blocks), dim3(256), 0, s, a.coords, a.M, a.S, sc.cursor, sc.key, sc.keyw);
  hipLaunchKernelGGL(constraint_rank_kernel, dim3((int)std::min<long long>((rows + 3) / 4, 65536)), dim3(256), 0, s, a.row_start,
                     rows, sc.key, sc.keyw, a.entry, a.entry_w);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

int constraint_loss_grad_launch(const ConstraintArgs& a, hipStream_t s) {
  ISHAP_REQUIRE(sizes_ok(a.npts, a.S), "constraint loss: 1 <= M <= 2^20 points and 2 <= S <= 1024");
  ISHAP_REQUIRE(a.planes && a.coords && a.gt && a.pw && a.row_start && a.entry && a.entry_w && a.dfeat && a.partials &&
                a.dplanes && a.loss, "null argument");
  ISHAP_REQUIRE(a.wsum > 0.f && a.wsum <= 3.0e38f, "constraint loss: the weights must have a positive finite sum");
  const long long ntiles = (a.npts + 31) / 32, rows = (long long)3 * a.S * a.S;
  ISHAP_TRY(ishap_set_max_lds((const void*)constraint_point_kernel, (int)MLP_SMEM));
  const int blocks = (int)std::min<long long>((ntiles + CONSTRAINT_WAVES - 1) / CONSTRAINT_WAVES, CONSTRAINT_MAX_BLOCKS);
  hipLaunchKernelGGL(constraint_point_kernel, dim3(blocks), dim3(64 * CONSTRAINT_WAVES), MLP_SMEM, s, a);
  hipLaunchKernelGGL(constraint_gather_kernel, dim3((unsigned)((rows + CONSTRAINT_GATHER_ROWS - 1) / CONSTRAINT_GATHER_ROWS)),
                     dim3(32 * CONSTRAINT_GATHER_ROWS), 0, s, a, rows, ntiles);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}
