// pixel_map.h -- mesh + camera -> the capture entries' two inputs (pixel_map.hip): the face normals and the pixel-to-face map.
//
// The projection is gluProject's arithmetic (model_view, then projection, both column-major as glGetDoublev returns them, then the
// perspective division and the viewport), every sum in the order the header include/brdf_levmar.h states, compiled with
// -ffp-contract=off: the device results have the bytes of the NumPy twins in brdf_amd/raster.py.
//
// One deviation from the reference's map (mode 0), on purpose: CalcPixel2SurfaceMapping (brdfdata.cpp:629-681) never checks the upper
// bound of a projected centroid and writes outside its image.  Here (int)winX >= W or (int)winY >= H writes nothing and is counted in
// stats[7].
#pragma once

#include <hip/hip_runtime.h>

namespace brdf {

constexpr int kPixelMapStats = 8;

// CalcFaceNormals (brdfdata.cpp:314-330): d_normals[nf][3] = normalize((v2 - v1) x (v3 - v1)); a vertex index outside [0, nv): NaN
int face_normals_run(const double *d_vertices, long long nv, const int *d_faces, long long nf, double *d_normals, hipStream_t stream);

struct PixelMapArgs {
  const double *d_vertices;  // [nv][3]
  long long nv;
  const int *d_faces;  // [nf][3]
  long long nf;  // both refused beyond INT_MAX
  const double *model_view, *projection, *viewport;  // host [16], [16], [4]
  int H, W;
  int mode;  // 0: the reference's map, one pixel per face centroid, the highest index wins; 1: rasterised and z-buffered
  int cull;  // mode 1: 1 drops the faces of negative window-space area
  int *d_pixel_map;    // [H][W]: face index or -1, row y = window row y (bottom-up)
  double *d_depth;     // [H][W] or null: the owner's window z, 2.0 where no face owns the pixel
  int *d_face_pixels;  // [nf] or null: the pixels each face owns
  long long *stats;    // host [kPixelMapStats] or null
  hipStream_t stream;
};
// Waits for the stream.  0, or kLmError with the error text.
int pixel_map_run(const PixelMapArgs &a);

}  // namespace brdf
