#pragma once
#include "common.h"

// Region-constrained drag edits: the weight map of the drag loss's mask term (csrc/drag.hip, the weighted gather pass) from 3-D
// regions.  A region is a union of boxes, spheres and one voxel grid; its SHADOW on triplane plane p is the set of plane texels
// it projects onto.  A plane texel stands for a whole column through the shape, so a region constrains its three shadows, not
// only its own volume.  Semantics: include/ishap.h, ishap_region_plane_weights.
struct RegionPrim {          // the layout of ishap_region_prim
  int kind;                  // 0 box, 1 sphere
  int role;                  // 0 keep, 1 free
  double a[3];               // box: lo; sphere: centre
  double b[3];               // box: hi; sphere: b[0] = radius
};
constexpr int REGION_MAX_D = 4096;
long long region_scratch_bytes(int W);
// weights_out [3][W][W]; counts (device int[2], may be null): texels of the keep / free shadows over the three planes before dilation
int region_plane_weights_launch(const RegionPrim* prims, int n_prims, const unsigned char* keep_vox, const unsigned char* free_vox,
                                int D, int W, int dilate, float keep_weight, float free_weight, float* weights_out, int* counts,
                                void* scratch, hipStream_t s);
// ABI 23.  marks_out uint8 [3][W][W]: bit 0 keep, bit 1 free, after dilation; scratch: region_scratch_bytes(W)
int region_plane_marks_launch(const RegionPrim* prims, int n_prims, const unsigned char* keep_vox, const unsigned char* free_vox, int D,
                              int W, int dilate, unsigned char* marks_out, int* counts, void* scratch, hipStream_t s);
// the feathered map (include/ishap.h, ishap_region_plane_feather); table: device double[table_len]
long long region_feather_scratch_bytes(int W);
int region_plane_feather_launch(const RegionPrim* prims, int n_prims, const unsigned char* keep_vox, const unsigned char* free_vox, int D,
                                int W, int dilate, float keep_weight, float free_weight, const double* table, int table_len,
                                float* weights_out, int* counts, void* scratch, hipStream_t s);
