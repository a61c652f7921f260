"""brdf_amd -- MI355X-native Levenberg-Marquardt BRDF fitter (the hot path of ccalantzis/BRDF).

The product is libbrdf_hip.so (C ABI in include/brdf_levmar.h, HIP kernels in brdf_amd/csrc).  This
package is the thin Python plumbing around it: ctypes bindings, torch tensors as device memory,
torch.distributed (RCCL) for the surfel-sharded multi-GPU driver, and the synthetic input generator.
"""
from . import synth  # noqa: F401
from ._lib import LIB_PATH, lib, last_error  # noqa: F401
from .fit import (METHOD_BC_DER, METHOD_BC_DIF, METHOD_DER, METHOD_DIF, MODEL_BLINN_PHONG, MODEL_PHONG, MODEL_WARD, FitResult, FitStats, fit_batch, fit_batch_multi, fit_stats_batch,  # noqa: F401
                  cosines, compact_samples, fit_capture, fit_capture_masked, fit_capture_single, fit_channels, fit_single, last_channels_stats, host_dlevmar, last_fit_stats, last_multi_stats, led_table, model_eval, chkjac, model_jacobian, set_launch_timing,
                  fit_batch_packed, fit_stats_batch_packed, last_packed_stats, pack_samples, last_batch_launch,
                  CaptureFaces, fit_capture_faces, group_capture_samples,
                  fit_batch_weighted, fit_stats_batch_weighted, CaptureMeans, LightMeans, fit_capture_means, capture_light_means,
                  CaptureSingleFaces, SingleSamples, fit_capture_single_faces, group_capture_single_samples,
                  ClippedFit, CaptureFacesClipped, SIGMA_MIN_8BIT, fit_batch_packed_clipped, fit_capture_faces_clipped, clip_samples, last_clip_stats,
                  CaptureMeansClipped, fit_capture_means_clipped, clip_light_means, initial_light_intervals,
                  FaceResiduals, CaptureLabelled, CaptureMaterials, LabelSamples, capture_face_residuals, fit_capture_labelled, fit_capture_materials,
                  group_capture_label_samples, assign_materials, seed_materials,
                  CaptureRender, CaptureRenderResiduals, RenderResidualsHost, capture_render, capture_render_residuals, surfaces_from_materials,
                  render_capture_host, render_residuals_host)
from . import raster  # noqa: F401
from .raster import (PixelMap, face_normals, face_normals_host, pixel_map, pixel_map_host, project_host, gl_frustum, gl_look_at, make_frustum,  # noqa: F401
                     parse_cal, tsai_camera)
from . import shadow  # noqa: F401
from .shadow import (AppliedVisibility, LightVisibility, apply_visibility, apply_visibility_host, light_visibility, light_visibility_host,  # noqa: F401
                     lit_matrix)
