// erase.hip — random erasing on a device fp32 batch [B][3][img][img] (include/vit_ops.h),
// and the host-only draw of the boxes (include/vit_trainer.h).
//
// The host validates every box, compacts the non-empty ones into a list of {image, k, box, noise stream
// seed} and uploads it with one small asynchronous copy from pinned staging; one launch then covers the
// batch: blockIdx.y = list entry, blockIdx.x = tile of the entry's 3 * h * w elements, lanes consecutive
// along x so that a wave's stores are runs of a box row.  The entry (and the mode) is uniform over a
// workgroup, so no switch diverges inside a wave.  Where boxes of one image overlap, a pixel belongs to
// the last box that covers it: every covered pixel is written once, whatever order workgroups run in.
// An image without a box gets no workgroup; a call without a box launches nothing.
//
// The normal of PIXEL and RAND mode is Box-Muller in double, rounded to fp32 once: every operation
// written here is one rounded double operation and no sum is present that could contract into an FMA,
// so the only freedom against the numpy statement is the last bits of the library's log and cos.
#include "erase.h"

#include <cmath>
#include <cstring>

#include "../../include/vit_trainer.h"
#include "common.h"

#pragma clang fp contract(off)

namespace vit {
namespace erase {

constexpr int T = 256;
constexpr int EPT = 4;  // elements per lane
constexpr int TILE = T * EPT;
constexpr int MAX_IMG = 8192;  // 3 * img^2 and every element index fit an int
constexpr int MAX_ENTRIES = 65535;  // gridDim.y

// the generator of the loaders' shuffle, vit_randaugment_draw and vit_drop_path_draw
__host__ __device__ __forceinline__ uint64_t sm64(uint64_t seed, uint64_t i) {
    uint64_t z = seed + (i + 1) * 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// z(p) of the noise stream sn (include/vit_ops.h)
__device__ __forceinline__ float normal_at(uint64_t sn, uint64_t p) {
    const uint64_t w = sm64(sn, p);
    const double u1 = (double)((w >> 40) + 1) * 0x1p-24;
    const double u2 = (double)((w >> 16) & 0xFFFFFFULL) * 0x1p-24;
    return (float)(sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2));
}

__global__ __launch_bounds__(T) void random_erase_k(float* __restrict__ pixels, const Entry* __restrict__ list, int img,
                                                     int entries, int mode) {
    const Entry e = list[blockIdx.y];  // uniform over the workgroup
    // the later boxes of the same image follow it in the list (at most three): a pixel they cover is theirs, so
    // every covered pixel is written once, by the last box that covers it (RAND: that box's colour)
    Entry later[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int q = min((int)blockIdx.y + 1 + j, entries - 1);
        later[j] = list[q];
        if (q <= (int)blockIdx.y || later[j].image != e.image) later[j].x1 = later[j].x0;  // none: an empty box
    }
    const int w = e.x1 - e.x0, hw = w * (e.y1 - e.y0), n = 3 * hw;
    const int base = (int)blockIdx.x * TILE;
    if (base >= n) return;  // the grid is sized for the largest box
    const int t = threadIdx.x;
    __shared__ float colour[3];
    if (mode == VIT_ERASE_RAND) {  // one colour per box and channel: three lanes of the workgroup, not every element
        if (t < 3) colour[t] = normal_at(e.sn, (uint64_t)(3 * img * img + 3 * e.k + t));
        __syncthreads();
    }
    float* im = pixels + (size_t)e.image * 3 * (size_t)img * (size_t)img;
#pragma unroll
    for (int j = 0; j < EPT; j++) {
        const int i = base + j * T + t;
        if (i >= n) break;
        const int c = i / hw, r = i - c * hw;
        const int y = r / w, x = r - y * w;
        const int ax = e.x0 + x, ay = e.y0 + y;
        bool theirs = false;
#pragma unroll
        for (int j = 0; j < 3; j++)
            theirs = theirs || (ax >= later[j].x0 && ax < later[j].x1 && ay >= later[j].y0 && ay < later[j].y1);
        if (theirs) continue;
        const int p = (c * img + ay) * img + ax;  // absolute position: < 3 * img^2
        float v = 0.0f;
        if (mode == VIT_ERASE_RAND) v = colour[c];
        else if (mode == VIT_ERASE_PIXEL) v = normal_at(e.sn, (uint64_t)p);
        im[p] = v;
    }
}

bool prepare(const int* boxes, int batch, int img, int max_count, int mode, unsigned long long seed,
             const long long* keys, const char* who, Plan& out) {
    if (!boxes || batch < 1 || img < 1 || img > MAX_IMG) {
        set_error("%s: bad arguments (boxes %p, batch %d, img %d of 1..%d)", who, (const void*)boxes, batch, img, MAX_IMG);
        return false;
    }
    if (max_count < 1 || max_count > 4) {
        set_error("%s: max_count %d outside 1..4", who, max_count);
        return false;
    }
    if (mode != VIT_ERASE_CONST && mode != VIT_ERASE_RAND && mode != VIT_ERASE_PIXEL) {
        set_error("%s: unknown mode %d", who, mode);
        return false;
    }
    if (mode != VIT_ERASE_CONST && !keys) {
        set_error("%s: the noise modes need host_keys", who);
        return false;
    }
    if ((long long)batch * max_count > MAX_ENTRIES) {
        set_error("%s: batch %d x max_count %d exceeds %d boxes", who, batch, max_count, MAX_ENTRIES);
        return false;
    }
    out.list.clear();
    out.batch = batch;
    out.img = img;
    out.mode = mode;
    out.tiles = 0;
    for (int b = 0; b < batch; b++)
        for (int k = 0; k < max_count; k++) {
            const int* q = boxes + ((size_t)b * max_count + k) * 4;
            const int x0 = q[0], y0 = q[1], x1 = q[2], y1 = q[3];
            if (x0 < 0 || y0 < 0 || x1 > img || y1 > img || x0 > x1 || y0 > y1) {
                set_error("%s: image %d box %d: [%d,%d) x [%d,%d) outside the %d x %d image", who, b, k, x0, x1, y0, y1,
                          img, img);
                return false;
            }
        }
    for (int b = 0; b < batch; b++) {
        const unsigned long long sn = keys ? seed ^ sm64(0x65726e6f697365ULL, (uint64_t)keys[b]) : 0ULL;  // "ernoise"
        for (int k = 0; k < max_count; k++) {
            const int* q = boxes + ((size_t)b * max_count + k) * 4;
            if (q[2] == q[0] || q[3] == q[1]) continue;  // empty
            out.list.push_back(Entry{b, k, q[0], q[1], q[2], q[3], sn});
            const int n = 3 * (q[2] - q[0]) * (q[3] - q[1]);
            const int tiles = (n + TILE - 1) / TILE;
            if (tiles > out.tiles) out.tiles = tiles;
        }
    }
    return true;
}

size_t list_bytes(int batch) { return (size_t)batch * 4 * sizeof(Entry); }

bool Stage::ensure(size_t need) {
    if (need <= bytes) return true;
    release();
    for (int i = 0; i < 2; i++)
        if (hipHostMalloc(&host[i], need, hipHostMallocDefault) != hipSuccess ||
            hipEventCreateWithFlags(&read[i], hipEventDisableTiming) != hipSuccess) {
            set_error("random erase: staging allocation (%zu bytes) failed", need);
            release();
            return false;
        }
    bytes = need;
    return true;
}

void Stage::release() {
    for (int i = 0; i < 2; i++) {
        if (read[i]) {
            (void)hipEventSynchronize(read[i]);
            (void)hipEventDestroy(read[i]);
        }
        if (host[i]) (void)hipHostFree(host[i]);
        read[i] = nullptr;
        host[i] = nullptr;
    }
    bytes = 0;
}

bool enqueue(const Plan& p, float* pixels, void* dev_list, Stage& stage, hipStream_t st) {
    if (p.list.empty()) return true;
    if (!pixels || !dev_list) {
        set_error("random erase: null device buffer");
        return false;
    }
    if (!stage.ensure(list_bytes(p.batch))) return false;
    const int k = stage.k & 1;
    stage.k++;
    const size_t bytes = p.list.size() * sizeof(Entry);
    VIT_HIP(hipEventSynchronize(stage.read[k]));  // the upload of two calls ago (done long since)
    memcpy(stage.host[k], p.list.data(), bytes);
    if (hipMemcpyAsync(dev_list, stage.host[k], bytes, hipMemcpyHostToDevice, st) != hipSuccess) {
        set_error("random erase: list upload failed");
        return false;
    }
    VIT_HIP(hipEventRecord(stage.read[k], st));
    const dim3 grid((unsigned)p.tiles, (unsigned)p.list.size());
    random_erase_k<<<grid, T, 0, st>>>(pixels, (const Entry*)dev_list, p.img, (int)p.list.size(), p.mode);
    count_hit(VIT_HIT_ERASE);
    if (hipGetLastError() != hipSuccess) {
        set_error("random erase: kernel launch failed");
        return false;
    }
    return !has_error();
}

}  // namespace erase
}  // namespace vit

using vit::set_error;
using namespace vit::erase;

extern "C" {

int vit_random_erase_draw(unsigned long long seed, long long key, int img, double prob, double min_area,
                          double max_area, double min_aspect, double max_aspect, int min_count, int max_count,
                          int* boxes, int* count) {
    if (!boxes || !count || img < 1) {
        set_error("vit_random_erase_draw: bad arguments (img %d)", img);
        return 1;
    }
    if (!(prob >= 0.0 && prob <= 1.0)) {
        set_error("vit_random_erase_draw: prob %g outside [0, 1]", prob);
        return 1;
    }
    if (!(min_area > 0.0 && min_area <= max_area && max_area <= 1.0)) {
        set_error("vit_random_erase_draw: areas %g, %g not 0 < min <= max <= 1", min_area, max_area);
        return 1;
    }
    if (!(min_aspect > 0.0 && min_aspect <= max_aspect && std::isfinite(max_aspect))) {
        set_error("vit_random_erase_draw: aspects %g, %g not 0 < min <= max", min_aspect, max_aspect);
        return 1;
    }
    if (min_count < 1 || min_count > max_count || max_count > 4) {
        set_error("vit_random_erase_draw: counts %d, %d not 1 <= min <= max <= 4", min_count, max_count);
        return 1;
    }
    const uint64_t s = (uint64_t)seed ^ sm64(0x6572617365ULL, (uint64_t)key);  // "erase"
    auto uni = [&](uint64_t pos) { return (double)(sm64(s, pos) >> 11) * 0x1p-53; };
    memset(boxes, 0, (size_t)max_count * 4 * sizeof(int));
    *count = 0;
    if (!(uni(0) < prob)) return 0;
    const int n = min_count + (int)std::floor(uni(1) * (double)(max_count - min_count + 1));
    *count = n;
    const double la = std::log(min_aspect), lb = std::log(max_aspect);
    for (int k = 0; k < n; k++)
        for (int a = 0; a < 10; a++) {
            const uint64_t at = 2 + (uint64_t)(k * 10 + a) * 4;
            const double target = (min_area + uni(at) * (max_area - min_area)) * ((double)img * (double)img) / (double)n;
            const double aspect = std::exp(la + uni(at + 1) * (lb - la));
            const int h = (int)std::rint(std::sqrt(target * aspect));
            const int w = (int)std::rint(std::sqrt(target / aspect));
            if (w < img && h < img) {
                const int top = (int)std::floor(uni(at + 2) * (double)(img - h + 1));
                const int left = (int)std::floor(uni(at + 3) * (double)(img - w + 1));
                int* q = boxes + 4 * k;
                q[0] = left;
                q[1] = top;
                q[2] = left + w;
                q[3] = top + h;
                break;
            }
        }
    return 0;
}

int vit_random_erase_f32(float* dev_pixels, int batch, int img, const int* host_boxes, int max_count, int mode,
                         unsigned long long seed, const long long* host_keys, void* stream) {
    if (!dev_pixels) {
        set_error("vit_random_erase_f32: null pixels");
        return 1;
    }
    Plan p;
    if (!prepare(host_boxes, batch, img, max_count, mode, seed, host_keys, "vit_random_erase_f32", p)) return 1;
    if (p.list.empty()) return 0;
    // this entry point's own list buffer and staging, per host thread (as vit_augment_u8's scratch); the
    // stream is the caller's choice, so a call on another stream first waits for the last one's kernel
    struct Scratch {
        void* list = nullptr;
        size_t bytes = 0;
        hipStream_t last = nullptr;
        bool used = false;
        Stage stage;
    };
    static thread_local Scratch sc;
    hipStream_t st = stream ? (hipStream_t)stream : vit::stream();
    if (sc.used && sc.last != st) VIT_HIP(hipStreamSynchronize(sc.last));
    const size_t need = list_bytes(batch);
    if (need > sc.bytes) {
        if (sc.list) (void)hipFree(sc.list);  // waits for the device
        sc.list = nullptr;
        sc.bytes = 0;
        if (hipMalloc(&sc.list, need) != hipSuccess) {
            sc.list = nullptr;
            set_error("vit_random_erase_f32: hipMalloc(%zu) failed", need);
            return 1;
        }
        sc.bytes = need;
    }
    sc.last = st;
    sc.used = true;
    const bool ok = enqueue(p, dev_pixels, sc.list, sc.stage, st);
    return ok && !vit::has_error() ? 0 : 1;
}

}  // extern "C"
