// erase.h — random erasing on a device fp32 batch (erase.hip), shared with the trainer (trainer.hip).
// include/vit_ops.h states the values; DESIGN.md §18 the design.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace vit {
namespace erase {

// one non-empty box as the kernel takes it, with the noise stream seed of its image
struct Entry {
    int image, k, x0, y0, x1, y1;
    unsigned long long sn;
};
static_assert(sizeof(Entry) == 32, "Entry layout");

// a validated call: the compacted list of non-empty boxes and the largest tile count among them
struct Plan {
    std::vector<Entry> list;
    int batch = 0, img = 0, mode = 0, tiles = 0;
};

// host only: validate every box of host_boxes [batch][max_count][4] and compact the non-empty ones.
// false + set_error("<who>: ...") on a bad argument; nothing has touched the GPU then.
bool prepare(const int* host_boxes, int batch, int img, int max_count, int mode, unsigned long long seed,
             const long long* host_keys, const char* who, Plan& out);
// device bytes of the list buffer for any call of this batch
size_t list_bytes(int batch);

// two pinned staging buffers for the list: enqueue() copies the list into one and uploads from it, so
// the call neither keeps the plan nor waits for the stream; a buffer is rewritten only after the upload
// that read it (two calls ago) has run
struct Stage {
    void* host[2]{};
    hipEvent_t read[2]{};
    size_t bytes = 0;
    int k = 0;
    bool ensure(size_t need);
    void release();
};

// upload p's list into dev_list and launch the kernel on st; pixels [batch][3][img][img] in place.
// An empty list does nothing at all.
bool enqueue(const Plan& p, float* pixels, void* dev_list, Stage& stage, hipStream_t st);

}  // namespace erase
}  // namespace vit
