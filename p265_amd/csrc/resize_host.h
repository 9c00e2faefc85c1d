// resize_host.h -- the host-only part of the scaled device-side output (p265r_batch_export_resized): validation
// of a p265r_resize_desc, the layout of an out_width x out_height frame, the position rule as a function and a
// scalar reference of the filters.  No HIP: p265r.hip calls it before anything is launched, and a CPU build
// (tools/resize_check.cpp) checks it on its own.
#pragma once
#include <stdint.h>
#include "export_host.h"
#include "resize_math.h"

namespace p265r {

// export_check_desc (desc->upsample ignored) plus the resize descriptor's own rules (P265R_EINVAL)
int resize_check_desc(const p265r_export_desc& d, const p265r_resize_desc& rs, int bit_depth, bool mono, ExportShape* s);
// the destination planes of one out_width x out_height frame
void resize_planes(const p265r_export_desc& d, const ExportShape& s, const p265r_resize_desc& rs, ExportPlane pl[3]);
// plane_off / pitch / frame_bytes against that frame, as export_check_layout
int resize_check_layout(const p265r_export_desc& d, const ExportShape& s, const p265r_resize_desc& rs, uint64_t* slot_bytes);
// a listed picture's crop window w x h against the filter (P265R_EINVAL: no sample, a window the arithmetic does
// not cover, P265R_RS_AREA with an output dimension above the window's)
int resize_check_window(const p265r_resize_desc& rs, int w, int h);
// the scale / bias the kernels apply to float outputs
void resize_norm(const p265r_resize_desc& rs, int bit_depth, float scale[3], float bias[3]);
// fp32 -> fp16 bits, round to nearest even
uint16_t resize_f16_bits(float f);

// Scalar reference of one plane.  src = the plane's window origin (uint16 samples, `stride` samples between rows);
// nw x nh = the LUMA window, mw x mh = the LUMA output size; chroma_plane: src is a chroma plane (nw / 2 x nh / 2
// samples); chroma_grid: the output is on the chroma grid (mw / 2 x mh / 2 samples, else mw x mh).  dst: tight.
int resize_plane_host(const uint16_t* src, uint64_t stride, int nw, int nh, int chroma_plane, int chroma_grid,
                      uint32_t filter, int mw, int mh, int32_t* dst);

}  // namespace p265r
