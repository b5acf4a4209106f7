#pragma once
#include "common.h"

// What the kernels of render.hip work on (api.hip fills it from the ABI arguments of ishap_render_mesh).
struct RenderCam {
  double eye[3], right[3], upv[3], fwd[3];   // orthonormal view basis: z_view = (p - eye) . fwd, positive in front of the eye
  double focal;                              // pixels per unit of x_view / z_view: (height / 2) / tan(fov_y / 2), square pixels
  double cx, cy;                             // width / 2, height / 2
  double near, far;
};
struct RenderArgs {
  const float* verts = nullptr;     // [nverts][3]
  const int* tris = nullptr;        // [ntris][3]
  const float* normals = nullptr;   // [nverts][3] or null: flat face normals
  const int* tri_part = nullptr;    // [ntris] or null: every triangle is part 0
  const float* parts = nullptr;     // [nparts][4]: r, g, b, lit
  long long nverts = 0, ntris = 0;
  int nparts = 0, width = 0, height = 0;
  RenderCam cam;
  void* scratch = nullptr;
  unsigned char* rgb = nullptr;     // [H][W][3] or null
  float* depth = nullptr;           // [H][W] or null
  int* tri_id = nullptr;            // [H][W] or null
};
constexpr int RENDER_MAX_SIDE = 16384;
long long render_scratch_bytes(long long nverts, long long ntris, int width, int height);   // -1: invalid sizes
int render_camera(const float* eye, const float* centre, const float* up, float fov_y_deg, float near, float far, int width,
                  int height, RenderCam& out);                                               // 0, or -2 with the error set
int render_mesh_launch(const RenderArgs& a, hipStream_t s);
int render_unproject_launch(const RenderCam& cam, const float* xyd, long long n, float* world, hipStream_t s);
