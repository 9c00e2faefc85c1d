// export_host.h -- the host-only part of the device-side output (p265r_batch_export): validation of
// a p265r_export_desc, the tight layout and the integer RGB coefficients.  No HIP: p265r.hip calls it
// before anything is launched, and a CPU build can check it on its own.
#pragma once
#include <stdint.h>
#include "../../include/p265r.h"

namespace p265r {

struct ExportShape {
    int es;             // bytes of one destination element
    int n_planes;       // destination planes: 3 planar / RGB planar, 2 semi-planar, 1 RGB packed
    int rgb;            // an RGB format
    int mono;           // the source is monochrome (4:0:0): planar has one plane, odd crops are legal except for
                        // semi-planar (whose CbCr plane is written as mid-grey)
};

struct ExportPlane {    // one destination plane of one cropped picture
    uint64_t row_bytes;
    int rows;
};

// enums, sample type against format and bit depth, crop parity (P265R_EINVAL)
// (mono: the source pictures are 4:0:0)
int export_check_desc(const p265r_export_desc& d, int bit_depth, ExportShape* s, bool mono = false);
// the planes of a pw x ph picture under d's crop; P265R_EINVAL when the crop leaves no sample
int export_planes(const p265r_export_desc& d, const ExportShape& s, int pw, int ph, ExportPlane pl[3]);
// plane_off / pitch / frame_bytes against a pw x ph picture: pitches, element alignment, overlap, slot
// size (P265R_EINVAL); *slot_bytes = the end of the slot's last plane
int export_check_layout(const p265r_export_desc& d, const ExportShape& s, int pw, int ph, uint64_t* slot_bytes);
// {cy, crr, cgb, cgr, cbb, yoff, 1 << (B - 1), D}
int export_coefficients(const p265r_export_desc& d, int bit_depth, int32_t out[8]);

}  // namespace p265r
