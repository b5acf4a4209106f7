#pragma once
#include "common.h"

// Exact squared Euclidean distance transform of a byte grid (csrc/edt.hip; include/ishap.h, ishap_edt).
constexpr int EDT_MAX_AXIS = 1024;       // the longest measured axis: a real distance stays below 2^22
constexpr int EDT_INF = 1 << 30;         // ISHAP_EDT_INF
// scratch bytes of a transform, -1 for sizes outside the limits
long long edt_scratch_bytes(int n0, int n1, int n2, int axes);
// the sizes are the caller's to check (ishap_edt does).  A voxel is a seed where (byte & mask) != 0 -- with invert, where it is
// 0 -- so a caller that keeps several sets in the bits of one byte grid (the region marks) transforms each without a copy.
int edt_launch(const unsigned char* seeds, unsigned mask, int n0, int n1, int n2, int axes, int invert, int* dist2, void* scratch,
               hipStream_t s);
