// The three rules every level-set extraction of the library shares (csrc/surface.hip on a dense volume, csrc/sparse_surface.hip
// on bricks): which side of the level a sample is on, where on a crossing edge the vertex sits, and the vertex's position.
// Both files compile these expressions and no others, so a vertex cut from a brick has the bits of the one cut from the volume.
#pragma once
#include "common.h"

// the tie rule: a sample AT the level is outside
__device__ __forceinline__ bool surf_inside(float value, float level) { return value - level > 0.f; }

// va, vb = value - level at the lower and at the upper end of a crossing edge -> the crossing's share of the edge
__device__ __forceinline__ float surf_edge_t(float va, float vb) { return va / (va - vb); }

// the vertex on the edge that leaves grid node (x, y, z) in direction (dx, dy, dz), in grid coordinates
__device__ __forceinline__ void surf_edge_vertex(float* __restrict__ out, int x, int y, int z, int dx, int dy, int dz, float t) {
  out[0] = (float)x + t * (float)dx;
  out[1] = (float)y + t * (float)dy;
  out[2] = (float)z + t * (float)dz;
}
