// light_visibility.h -- cast shadows (light_visibility.hip): which lights each face's centre can see, and that visibility painted into
// the images every capture entry reads.
//
// The definitions are include/brdf_levmar.h's; every sum in the order stated there, compiled with -ffp-contract=off: the device results
// have the bytes of the NumPy twins in brdf_amd/shadow.py.  The reference has nothing to compare with: its voxel-grid shadow code in
// brdfdata.cpp is commented out.
#pragma once

#include <hip/hip_runtime.h>

namespace brdf {

constexpr int kVisibilityStats = 5;  // valid faces, invalid faces, (face, light) pairs facing away, pairs lit, pairs shadowed
constexpr int kVisibilityMaxL = 64;  // one bit of a 64-bit word per light

struct LightVisibilityArgs {
  const double *d_vertices;  // [nv][3]
  long long nv;
  const int *d_faces;  // [nf][3]
  long long nf;  // both refused beyond INT_MAX
  const double *d_normals;  // [nf][3] or null: with normals a pair with !(n . d > 0) faces away
  const double *leds;       // host [L][3]
  int L;                    // 1 ... 64
  double t_min;             // [0, 0.5): a hit needs t_min A < T < (1 - t_min) A
  unsigned long long *d_face_lit;  // [nf]: bit l set iff light l is visible from the face's centre
  long long *stats;                // host [kVisibilityStats] or null
  hipStream_t stream;
};
// Waits for the stream.  0, or kLmError with the error text.
int light_visibility_run(const LightVisibilityArgs &a);

struct ApplyVisibilityArgs {
  const unsigned char *d_images;  // [L][H][W][3]
  int L, H, W;
  const int *d_pixel_map;  // [H][W]
  const unsigned long long *d_face_lit;  // [nf]
  int nf;
  int level;  // 0 ... 255: what a shadowed pixel's three bytes become
  unsigned char *d_out;  // [L][H][W][3]: d_images itself (in place: only painted bytes are written) or a buffer apart from it
  unsigned long long *d_shadowed;  // [L] or null: painted pixels per light
  hipStream_t stream;
};
// Enqueues and returns.  0, or kLmError with the error text.
int apply_visibility_run(const ApplyVisibilityArgs &a);

}  // namespace brdf
