// capture_materials.h -- K materials per object (capture_materials.hip): the carried faces' residuals against M candidate materials in
// one read of the samples, one fit per (label, channel) over the samples of the faces that carry the label, and Lloyd's iteration
// around the two.  The argument structs are capture_fit.h's; what the three entries share besides is here.
#pragma once

#include "capture_fit.h"

namespace brdf {

constexpr int kMaterialRoundsMax = 64;  // brdf_hip_fit_capture_materials_dev: rounds in [0, kMaterialRoundsMax]

int capture_face_residuals_run(const CaptureResidualsArgs &a);  // refuses bad arguments before any HIP call
int capture_labelled_run(const CaptureLabelledArgs &a);         // refuses bad arguments before any HIP call
int capture_materials_run(const CaptureMaterialsArgs &a);       // refuses bad arguments before any HIP call

}  // namespace brdf
