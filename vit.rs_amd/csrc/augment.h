// augment.h — RandAugment on the device uint8 batch (augment.hip), shared with the trainer's staging
// (trainer.hip) and the JPEG loader's device half (jpeg.hip).  include/vit_data.h states the ops.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/vit_data.h"

namespace vit {
namespace aug {

// one op as the kernels take it: the affine coefficients already in Pillow's 16.16 fixed point
// (fx[2], fx[5] include the half-pixel terms), and which buffer holds the image when the op runs
struct DevOp {
    int op, iarg;
    float farg;
    int src;  // 0 = the caller's images, 1 = the scratch copy (after an odd number of out-of-place ops)
    int fx[6];
};
constexpr int OP_COPY_BACK = VIT_AUG_NUM_OPS;  // scratch -> images, after the last slot

// a validated plan in device form: [batch][depth + 1] ops (the last column is the copy back) and
// which launches each slot needs
struct Prepared {
    std::vector<DevOp> ops;
    int batch = 0, img = 0, depth = 0;
    unsigned char fill[3]{};
    bool lut[VIT_AUG_MAX_DEPTH + 1]{}, inplace[VIT_AUG_MAX_DEPTH + 1]{}, outplace[VIT_AUG_MAX_DEPTH + 1]{};
};

// host only: validate host_plan [batch][depth] (include/vit_data.h) and convert it.  false +
// set_error("<who>: ...") on an invalid plan.
bool prepare(const vit_aug_op_t* host_plan, int batch, int img, int depth, const unsigned char* fill3,
             const char* who, Prepared& out);
// device bytes enqueue() needs for a batch of `batch` img x img images (any depth)
size_t scratch_bytes(int batch, int img);
// upload p's ops and launch its kernels on st; images [batch][img][img][3] in place.  p.ops is read
// by the upload: keep p unchanged until st has passed that point (read, if given, is recorded
// right after the upload).
bool enqueue(const Prepared& p, uint8_t* images, void* scratch, hipStream_t st, hipEvent_t read = nullptr);

}  // namespace aug
}  // namespace vit
