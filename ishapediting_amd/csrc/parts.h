#pragma once
#include "regions.h"

// Part edits: from a region and a rigid motion to handles, targets and free regions (csrc/parts.hip; semantics: include/ishap.h,
// ishap_region_select / ishap_region_handles / ishap_region_transform).  All arithmetic is integer or double.
constexpr int PARTS_MAX_D = 1024;            // a voxel's coordinates pack into 3 x 10 bits, its linear index stays below 2^30
constexpr int PARTS_MAX_HANDLES = 4096;
struct PartsRigid {                          // the 15 host doubles of ishap_region_transform
  double R[9];                               // row-major rotation
  double pivot[3];
  double t[3];
};
