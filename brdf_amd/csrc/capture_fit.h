// capture_fit.h -- the capture entries' host interface: what capi.hip fills and calls.  The seven entries share one description of the
// capture (CaptureArgs); the per-face entries share the validity rule and what the grouping writes (CaptureGrouped).
#pragma once

#include <hip/hip_runtime.h>

namespace brdf {

// vectors -> cosines (cosines.hip)
int cosines_run(const double *d_vertices, const int *d_faces, const double *d_normals, const int *d_surfels, long long S,
                const double *leds, int L, const double *view, int rv_mode, double *d_angles, hipStream_t stream);
void led_table(double *out16x3);

// what every capture entry takes: the capture, the mesh, the rig, the fit's settings and the stream
struct CaptureArgs {
  int model;
  const unsigned char *d_images;  // [L][H][W][3], BGR
  int L, H, W;
  const int *d_pixel_map;  // [H][W]: the face under the pixel; outside [0, nf): background
  const double *d_vertices;
  const int *d_faces;
  const double *d_normals;
  int nf;
  const double *leds, *view;  // host [L][3], [3]
  int rv_mode;
  const double *p0, *lb, *ub;  // host [3] (lb, ub: or null)
  int itmax;
  const double *opts;  // host [5] or null
  hipStream_t stream;
};

// the validity rule of brdf_hip_fit_capture_masked_dev: sample i of a fit takes part iff v_min <= 8-bit intensity <= v_max and every
// cosine plane the model reads is > cos_min; d_surface_count[nf][3] (device, or null) receives the stored fits' sample counts
struct CaptureMask {
  int v_min, v_max;
  double cos_min;
  int *d_surface_count;
};

// the pixel loop of CalcBRDFEquation (capture_fit.hip): brdf_hip_fit_capture_dev, _stats_dev (a statistics map is asked for) and
// _masked_dev (mask: a validity rule, a ragged fit)
struct CaptureFitArgs {
  CaptureArgs cap;
  double *d_brdf_surfaces;  // [nf][3][3]
  double *avg;              // host [3] or null
  long long *n_pixels;      // host or null
  double *d_surface_covar, *d_surface_stats;  // [nf][3][9], [nf][3][kStatsSz] or null: the optional statistics tail
  int *d_surface_rank;                        // [nf][3] or null
  const CaptureMask *mask;                    // or null
};
int capture_fit_run(const CaptureFitArgs &a);

// brdf_hip_fit_capture_single_dev (capture_fit.hip): one fit per channel over the L samples of every carried face's last pixel
struct CaptureSingleArgs {
  CaptureArgs cap;
  double *single_brdf;      // host [3][3]
  double *info;             // host [3][10] or null
  long long *n_faces_used;  // host or null
};
int capture_fit_single_run(const CaptureSingleArgs &a);

// what the per-face entries share: the capture, the rule (as CaptureMask) and what the grouping writes (capture_group.hip)
struct CaptureGrouped {
  CaptureArgs cap;
  int v_min, v_max;
  double cos_min;
  int *d_face_pixels;             // [nf] or null
  long long *n_pixels, *n_faces;  // host or null
};

// brdf_hip_fit_capture_faces_clipped_dev: the sigma clip of the per-face fits (clip_fit.h) and its two maps
struct CaptureClip {
  double kappa, sigma_min;
  int rounds;
  int *d_surface_kept, *d_surface_rounds;  // [nf][3] or null: the returned set's size, rounds_used
};

// brdf_hip_fit_capture_faces_dev (capture_faces.hip): one fit per (face, channel) over the valid samples of all the face's pixels,
// through the packed batch
struct CaptureFacesArgs {
  CaptureGrouped g;
  long long workspace_bytes;  // the packed calls'
  double *d_brdf_surfaces;    // [nf][3][3]
  double *d_surface_info;     // [nf][3][10] or null
  int *d_surface_ret;         // [nf][3] or null
  double *d_surface_covar, *d_surface_stats;  // [nf][3][9], [nf][3][kStatsSz] or null
  int *d_surface_rank, *d_surface_count;      // [nf][3] or null
  double *avg;                                // host [3] or null
  const CaptureClip *clip = nullptr;          // null: brdf_hip_fit_capture_faces_dev; otherwise the clipped entry, under its own name
};
int capture_faces_run(const CaptureFacesArgs &a);  // refuses bad arguments before any HIP call

// brdf_hip_fit_capture_means_clipped_dev: the sigma clip of the means capture (capture_means_clip.h) and its four maps
struct CaptureMeansClip {
  CaptureClip clip;
  unsigned char *d_surface_vlo, *d_surface_vhi;  // [nf][3][L] or null: the returned set's grey-level interval per light
};

// brdf_hip_fit_capture_means_dev (capture_means.hip): the per-face capture as a weighted fit of per-light means
struct CaptureMeansArgs {
  CaptureFacesArgs faces;  // brdf_hip_fit_capture_faces_dev's arguments (workspace_bytes unused; d_surface_count receives k)
  int *d_surface_lights;   // [nf][3] or null: the lights with a sample, the weighted fit's n
  const CaptureMeansClip *clip = nullptr;  // null: brdf_hip_fit_capture_means_dev; otherwise the clipped entry, under its own name
};
int capture_means_run(const CaptureMeansArgs &a);  // refuses bad arguments before any HIP call

// brdf_hip_fit_capture_single_faces_dev (capture_single_faces.hip): ONE fit per channel over the valid samples of every pixel of every
// carried face, through the single-fit path, and the carried faces' sums of squared residuals against that fit.
struct CaptureSingleFacesArgs {
  CaptureGrouped g;
  double *single_brdf;   // host [3][3], required
  double *info;          // host [3][10] or null
  int *ret;              // host [3] or null
  double *covar, *stats;  // host [3][9], [3][kStatsSz] or null
  int *rank;              // host [3] or null
  long long *count;       // host [3] or null: the samples of channel c's fit
  double *d_face_sumsq;   // [nf][3] or null
  int *d_face_count;      // [nf][3] or null
};
int capture_single_faces_run(const CaptureSingleFacesArgs &a);  // refuses bad arguments before any HIP call; the channels with ret < 0

// brdf_hip_capture_face_residuals_dev (capture_materials.hip): the carried faces' sums of squared residuals against M materials
struct CaptureResidualsArgs {
  CaptureGrouped g;           // (p0, lb, ub, itmax, opts unused: no fit)
  const double *d_materials;  // [M][3][3], required
  int M;
  double *d_face_sumsq;       // [nf][M][3] or null
  int *d_face_count;          // [nf][3] or null
};

// brdf_hip_fit_capture_labelled_dev (capture_materials.hip): one fit per (label, channel) over the faces that carry the label
struct CaptureLabelledArgs {
  CaptureGrouped g;           // (p0 unused: the materials are the starting points)
  long long workspace_bytes;  // the packed calls'
  int *d_face_label;          // [nf], required, read only here; outside [0, K): the face takes part in nothing
  int K;
  double *d_materials;        // [K][3][3] in/out, required
  double *d_info;             // [K][3][10] or null
  int *d_ret;                 // [K][3] or null
  double *d_covar, *d_stats;  // [K][3][9], [K][3][kStatsSz] or null
  int *d_rank, *d_count;      // [K][3] or null
  int *d_label_faces;         // [K] or null: the carried faces of the label
};

// brdf_hip_fit_capture_materials_dev (capture_materials.hip): assign, refit, until no label moves
struct CaptureMaterialsArgs {
  CaptureLabelledArgs fit;  // d_face_label: written, [nf], required
  int rounds;               // refits at most
  double *d_face_sumsq;     // [nf][3] or null: against the face's own material
  int *d_face_count;        // [nf][3] or null
  int *rounds_used, *settled;  // host or null
  long long *changed;          // host [rounds + 1] or null: the faces whose label changed, per assignment (-1: no such assignment)
};

// brdf_hip_capture_render_dev (capture_render.hip): the model at the fitted surfaces under `L` lights of any kind, as a value table
// and as 8-bit images in the captures' layout
struct CaptureRenderArgs {
  CaptureArgs cap;  // (d_images, p0, lb, ub, itmax, opts unused: no capture is read, no fit)
  const double *d_brdf_surfaces;  // [nf][3][3], required
  int background;                 // -1: pixels that carry no face are left untouched; otherwise their grey level
  double *d_face_values;          // [nf][3][L] or null
  unsigned char *d_rendered;      // [L][H][W][3] or null
};
int capture_render_run(const CaptureRenderArgs &a);  // refuses bad arguments before any HIP call

// brdf_hip_capture_render_residuals_dev (capture_render.hip): the captures minus the rendered grey levels, as integer maps
struct CaptureRenderResidualsArgs {
  CaptureGrouped g;  // (p0, lb, ub, itmax, opts, d_face_pixels, n_faces unused)
  const double *d_brdf_surfaces;  // [nf][3][3], required
  long long *d_light_count, *d_light_sum, *d_light_sumsq;  // [L][3] or null
  int *d_face_light_count;                                 // [nf][3][L] or null
  long long *d_face_light_sum, *d_face_light_sumsq;        // [nf][3][L] or null
  unsigned char *d_abs_max, *d_worst_light;                // [H][W][3] at map coordinates, or null
  double *d_face_values;                                   // [nf][3][L] or null
};
int capture_render_residuals_run(const CaptureRenderResidualsArgs &a);  // refuses bad arguments before any HIP call

// brdf_hip_surfaces_from_materials_dev (capture_render.hip): surfaces[f] = materials[label[f]], `fill` where the label is outside [0, K)
struct SurfacesFromMaterialsArgs {
  const int *d_face_label;  // [nf]
  int nf;
  const double *d_materials;  // [K][3][3]
  int K;
  const double *fill;       // host [3]
  double *d_brdf_surfaces;  // [nf][3][3]
  hipStream_t stream;
};
int surfaces_from_materials_run(const SurfacesFromMaterialsArgs &a);  // refuses bad arguments before any HIP call

}  // namespace brdf
