// Handle tracking: after a guided step, where is each drag handle now?  DragGAN's point tracking (the second half of the motion
// supervision the drag loss follows) in the feature space the loss itself reads: a nearest-neighbour search, in L1 over a small
// patch of lattice positions, of the guidance tap's features AT the handle among the edited tap's features AROUND it.
// The definition is DESIGN.md 5.2l; the tap layout, plane_axes, the channel gather and the bilinear sample are those of drag.hip
// (drag.h), so the candidate K_in + k = 0 reads the same bits as the source lattice and a tap equal to its guidance has D = 0.
//
// The search is separable: D(b; kx, ky, kz) = D_0(kx, ky) + D_1(ky, kz) + D_2(kx, kz), one 2-D map of (2R+1)^2 sums per plane.
//   stage 1, track_corr_kernel: a workgroup (16 waves) per (handle, plane, channel chunk).  It samples the guidance tap at the (2rp+1)^2
//     patch positions and the edited tap ONCE at each of the (2(R+rp)+1)^2 positions any candidate's patch can touch, into LDS
//     (fp32, [position][channel]: lanes run over channels, contiguous in NHWC and conflict-free in LDS), then a wave per
//     candidate adds |E - O| over the patch and its channels.
//   stage 2, track_argmin_kernel: a workgroup per handle adds the chunks of each map, forms the (2R+1)^3 sums and takes the
//     argmin under the tie rule (smallest D, then smallest |k|^2, then lowest linear index).
// No float atomics, one fixed summation order: D is bitwise repeatable and a handle's result does not depend on which other
// handles or edits share the launch (every workgroup reads its own handle and writes its own slice).
//
// The addition chain of one D (tests/test_gpu_track.py derives its tolerance from it): a lane adds its ceil(P / nsub) patch terms in
// order (P = (2rp+1)^2, nsub = 64 / chunk width lanes share a channel), 6 butterfly levels add the 64 lanes, nchunk chunk sums
// are added in order, 2 additions join the three planes: n = ceil(P / nsub) + 6 + nchunk + 2.
#include "track.h"

int track_chunk_width(int R, int rp) {
  const int sE = 2 * (R + rp) + 1, sO = 2 * rp + 1;
  for (int cw = 64; cw > 16; cw >>= 1)
    if ((sE * sE + sO * sO) * cw * (int)sizeof(float) <= TRACK_LDS_BYTES) return cw;
  return 16;       // R = 8, rp = 4: 706 positions * 16 channels * 4 bytes = 45184
}

static bool track_range_ok(int R, int rp) { return R >= 0 && R <= TRACK_MAX_R && rp >= 0 && rp <= TRACK_MAX_RP; }

long long track_scratch_bytes(int Btot, int R, int rp, int Cc) {
  if (Btot < 1 || Cc < 1 || !track_range_ok(R, rp)) return -1;
  const int side = 2 * R + 1;
  const long long n = (long long)Btot * 3 * ceil_div(Cc, track_chunk_width(R, rp)) * side * side * (long long)sizeof(float);
  return (n + 15) & ~15ll;
}

__device__ __forceinline__ int track_edit_of(const TrackArgs& a, int h) {
  int e = 0;
  while (e + 1 < a.E && h >= a.hoff[e + 1]) ++e;       // workgroup-uniform
  return e;
}

// CW: channels of a chunk (64, 32 or 16); 64 / CW lanes share a channel and split the patch positions between them
constexpr int TRACK_U = 4;
// 16 waves: the kernel is a chain of short dependent steps (texel loads, then LDS reads) on few workgroups -- 9 for one handle at
// the default search -- so its time is the length of one workgroup's chain, which the waves divide between them
constexpr int TRACK_THREADS = 1024;
template <int CW>
__global__ __launch_bounds__(TRACK_THREADS) void track_corr_kernel(TrackArgs a, int nchunk) {
  extern __shared__ float track_lds[];       // [nE + nO][CW]: the edited tap's window, then the guidance patch
  const int sideE = 2 * (a.R + a.rp) + 1, sideO = 2 * a.rp + 1, side = 2 * a.R + 1;
  const int nE = sideE * sideE, nO = sideO * sideO;
  const int chunk = blockIdx.x % nchunk, p = (blockIdx.x / nchunk) % 3, h = blockIdx.x / (3 * nchunk);
  const int e = track_edit_of(a, h);
  int ac, ar;
  plane_axes(p, ac, ar);
  const float su = a.sources[h * 3 + ac], sv = a.sources[h * 3 + ar];
  const int mc0 = a.K_in[h * 3 + ac] - a.R - a.rp, mr0 = a.K_in[h * 3 + ar] - a.R - a.rp;   // lattice index of the window's corner
  const half_t* ed = a.edit + (long long)e * a.W * a.W * a.ld;
  const half_t* og = a.orig + e * a.orig_stride;
  // TRACK_THREADS is a multiple of CW: a thread keeps one channel through the whole fill
  const int c = chunk * CW + (threadIdx.x % CW);
  const bool live = c < a.Cc;
  const int ch = live ? a.chmap[p * a.Cc + c] : 0;
  // TRACK_U samples per trip: all their texel loads are issued before the first is used (the load-ordering rule of
  // drag_motion_body).  Every load is unconditional at a clamped coordinate; a tap outside the map (zeros padding), a dead channel
  // and a slot past the end enter with value 0 and weight 0, whatever the clamped texel holds.
  const int total = (nE + nO) * CW;
  for (int it0 = threadIdx.x; it0 < total; it0 += TRACK_THREADS * TRACK_U) {
    half_t tv[TRACK_U][4];
    float tw[TRACK_U][4];
#pragma unroll
    for (int u = 0; u < TRACK_U; ++u) {
      const int it = it0 + TRACK_THREADS * u;
      const bool on = live && it < total;
      const int pos = min(it, total - 1) / CW;
      const bool isO = pos >= nE;
      const int q = isO ? pos - nE : pos, sd = isO ? sideO : sideE;
      const int j = q / sd, i = q - j * sd;
      const int mc = isO ? i - a.rp : mc0 + i, mr = isO ? j - a.rp : mr0 + j;
      const half_t* tap = isO ? og : ed;
      const Bilin b = bilin_setup(lattice(su, a.voxel, mc), lattice(sv, a.voxel, mr), a.W);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int x = b.x0 + (k & 1), y = b.y0 + (k >> 1);
        const int xc = min(max(x, 0), a.W - 1), yc = min(max(y, 0), a.W - 1);
        const half_t v = tap[((long long)yc * a.W + xc) * a.ld + ch];
        const bool in = on && x == xc && y == yc;
        tv[u][k] = in ? v : (half_t)0.f;
        tw[u][k] = in ? b.w[k] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < TRACK_U; ++u) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) s = __fmaf_rn(tw[u][k], (float)tv[u][k], s);      // the fma chain of drag_motion_body, both sides
      if (it0 + TRACK_THREADS * u < total) track_lds[it0 + TRACK_THREADS * u] = s;
    }
  }
  __syncthreads();
  const float* sE = track_lds;
  const float* sO = track_lds + nE * CW;
  constexpr int NSUB = 64 / CW;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int cl = lane % CW, sub = lane / CW;
  float* out = a.partial + ((long long)(h * 3 + p) * nchunk + chunk) * side * side;
  for (int cand = wave; cand < side * side; cand += TRACK_THREADS / 64) {
    const int kr = cand / side, kc = cand - kr * side;      // candidate offset + R along the row / the column axis
    float acc = 0.f;
    int j = sub / sideO, i = sub - j * sideO;             // patch position q = j * sideO + i, walked without a division
#pragma unroll 4
    for (int q = sub; q < nO; q += NSUB) {
      acc += fabsf(sE[((kr + j) * sideE + kc + i) * CW + cl] - sO[q * CW + cl]);
      i += NSUB;
      while (i >= sideO) { i -= sideO; ++j; }
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) out[cand] = acc;
  }
}

struct TrackBest { float d; int r2, idx; };
__device__ __forceinline__ bool track_better(const TrackBest& x, const TrackBest& y) {
  return x.d < y.d || (x.d == y.d && (x.r2 < y.r2 || (x.r2 == y.r2 && x.idx < y.idx)));
}

__global__ __launch_bounds__(256) void track_argmin_kernel(TrackArgs a, int nchunk) {
  constexpr int SMAX = 2 * TRACK_MAX_R + 1;
  __shared__ float dm[3 * SMAX * SMAX];
  __shared__ TrackBest red[4];
  const int h = blockIdx.x, R = a.R, side = 2 * R + 1, s2 = side * side, s3 = s2 * side;
  const float* part = a.partial + (long long)h * 3 * nchunk * s2;
  for (int t = threadIdx.x; t < 3 * s2; t += 256) {
    const int p = t / s2, cand = t - p * s2;
    const float* src = part + (long long)p * nchunk * s2 + cand;
    float s = src[0];
    for (int q = 1; q < nchunk; ++q) s += src[(long long)q * s2];
    dm[t] = s;
  }
  __syncthreads();
  const int centre = (R * side + R) * side + R;
  TrackBest best = {__builtin_inff(), 0x7fffffff, 0x7fffffff};      // loses to every candidate with a D that is not NaN
  for (int idx = threadIdx.x; idx < s3; idx += 256) {
    const int x = idx % side, y = (idx / side) % side, z = idx / s2;       // k + R
    const float d = (dm[y * side + x] + dm[s2 + z * side + y]) + dm[2 * s2 + z * side + x];
    if (a.volume) a.volume[(long long)h * s3 + idx] = d;
    if (idx == centre) a.dist0[h] = d;
    const TrackBest cur = {d, (x - R) * (x - R) + (y - R) * (y - R) + (z - R) * (z - R), idx};
    if (track_better(cur, best)) best = cur;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const TrackBest oth = {__shfl_xor(best.d, o), __shfl_xor(best.r2, o), __shfl_xor(best.idx, o)};
    if (track_better(oth, best)) best = oth;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w)
      if (track_better(red[w], best)) best = red[w];
    if (best.idx == 0x7fffffff) { best.idx = centre; best.d = (dm[R * side + R] + dm[s2 + R * side + R]) + dm[2 * s2 + R * side + R]; }   // every D NaN: stay
    const int x = best.idx % side, y = (best.idx / side) % side, z = best.idx / s2;
    a.K_out[h * 3 + 0] = a.K_in[h * 3 + 0] + x - R;
    a.K_out[h * 3 + 1] = a.K_in[h * 3 + 1] + y - R;
    a.K_out[h * 3 + 2] = a.K_in[h * 3 + 2] + z - R;
    a.dist[h] = best.d;
  }
}

int track_launch(const TrackArgs& a, hipStream_t s) {
  ISHAP_REQUIRE(a.E >= 1 && a.E <= DRAG_MAX_EDITS, "drag track: E must be in 1..32");
  ISHAP_REQUIRE(a.R >= 0 && a.R <= TRACK_MAX_R, "drag track: R must be in 0..8");
  ISHAP_REQUIRE(a.rp >= 0 && a.rp <= TRACK_MAX_RP, "drag track: rp must be in 0..4");
  ISHAP_REQUIRE(a.W > 1 && a.ld >= 1 && a.Cc >= 1 && a.orig_stride >= 0, "drag track: dims");
  ISHAP_REQUIRE(a.hoff[0] == 0, "drag track: handle_offsets[0] must be 0");
  for (int e = 0; e < a.E; ++e) ISHAP_REQUIRE(a.hoff[e + 1] > a.hoff[e], "drag track: every edit needs at least one handle");
  const int Btot = a.hoff[a.E];
  const int cw = track_chunk_width(a.R, a.rp), nchunk = ceil_div(a.Cc, cw);
  ISHAP_REQUIRE((long long)Btot * 3 * nchunk < (1ll << 30), "drag track: too many handles");
  const int sE = 2 * (a.R + a.rp) + 1, sO = 2 * a.rp + 1;
  const size_t lds = (size_t)(sE * sE + sO * sO) * cw * sizeof(float);
  const dim3 grid((unsigned)(Btot * 3 * nchunk)), block(TRACK_THREADS);
  if (cw == 64) hipLaunchKernelGGL(track_corr_kernel<64>, grid, block, lds, s, a, nchunk);
  else if (cw == 32) hipLaunchKernelGGL(track_corr_kernel<32>, grid, block, lds, s, a, nchunk);
  else hipLaunchKernelGGL(track_corr_kernel<16>, grid, block, lds, s, a, nchunk);
  hipLaunchKernelGGL(track_argmin_kernel, dim3((unsigned)Btot), dim3(256), 0, s, a, nchunk);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}
