// Generalized winding number launches shared inside the library (csrc/winding.hip); the C ABI is in include/ishap.h.
#pragma once
#include "common.h"

// device bytes the part sums of (nprims primitives, npts queries) need; a multiple of 256, never 0; -1 on invalid sizes
long long ishap_winding_bytes(long long nprims, long long npts);
// out[i] = w(pts[i]) of the triangle mesh (binary 0), or the 0/1 inside flag w > 0.5 (binary +1) / w < -0.5 (binary -1);
// arguments are the caller's to check
void ishap_winding_launch_mesh(const float* verts, const int* tris, long long ntris, const float* pts, long long npts, float* out,
                               int binary, void* scratch, hipStream_t s);
