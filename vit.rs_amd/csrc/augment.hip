// augment.hip — RandAugment on the device uint8 batch [B][img][img][3] (include/vit_data.h).
//
// The host validates the plan, computes everything that needs trigonometry or doubles of its own
// (Pillow's 16.16 fixed-point affine coefficients) and decides which launches a slot needs; the
// device applies integers, fp32 blends and the fixed-point map.  Per plan slot, over the whole batch:
//   aug_lut_k       one workgroup per image whose op is a per-value table (autocontrast, equalize,
//                   posterize, solarize, brightness, contrast): per-wave 3 x 256 histograms or the
//                   luma sum with integer LDS atomics (order-independent, so deterministic), then
//                   the image's [3][256] uint8 table
//   aug_inplace_k   table lookup (16 bytes per lane), colour blend (16 pixels per lane), or the
//                   final copy back of images that ended in the scratch buffer
//   aug_outplace_k  sharpness and the affine ops, one pixel per lane, from the buffer that holds the
//                   image into the other one (the host tracks which, per image)
// Every image's op is uniform over its workgroups (blockIdx.y = image), so the switch on the op
// never diverges inside a wave.  Identity launches nothing.
#include "augment.h"

#include <cmath>
#include <cstring>

#include "common.h"

// blends and the smoothing sum are stated operation by operation (each rounded): no fused multiply-add
#pragma clang fp contract(off)

namespace vit {
namespace aug {

constexpr int T = 256;
constexpr int MAX_IMG = 8192;

// ------------------------------------------------------------------------------ device helpers
__device__ __forceinline__ int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// Image.blend(degenerate d, image v, f)
__device__ __forceinline__ uint8_t blend_u8(float d, float v, float f, bool convex) {
    float t = d + f * (v - d);
    if (!convex) t = fminf(fmaxf(t, 0.f), 255.f);
    return (uint8_t)(int)t;
}

__device__ __forceinline__ bool is_lut_op(int op) {
    return op == VIT_AUG_AUTOCONTRAST || op == VIT_AUG_EQUALIZE || op == VIT_AUG_POSTERIZE ||
           op == VIT_AUG_SOLARIZE || op == VIT_AUG_BRIGHTNESS || op == VIT_AUG_CONTRAST;
}

// The 16-byte chunks covering the n bytes at p: chunk k holds the image bytes [16 k - head, 16 k - head + 16)
// with head = p & 15, so that every full chunk is a 16-byte-aligned address whatever p is (n is odd
// for odd img, so images after the first start anywhere).
__device__ __forceinline__ int chunk_head(const void* p) { return (int)((uintptr_t)p & 15); }
__host__ __device__ __forceinline__ int max_chunks(int n) { return (n + 15 + 15) / 16; }

// ------------------------------------------------------------------------------ tables
__global__ __launch_bounds__(T) void aug_lut_k(const uint8_t* __restrict__ images, const uint8_t* __restrict__ alt,
                                                const DevOp* __restrict__ ops, int stride, int slot, int npix,
                                                uint8_t* __restrict__ luts) {
    const int b = blockIdx.x, t = threadIdx.x;
    const DevOp o = ops[(size_t)b * stride + slot];
    if (!is_lut_op(o.op)) return;  // uniform over the workgroup
    uint8_t* lut = luts + (size_t)b * 768;
    if (o.op == VIT_AUG_POSTERIZE) {
        const uint8_t v = (uint8_t)(t & ~((1 << (8 - o.iarg)) - 1));
        lut[t] = lut[256 + t] = lut[512 + t] = v;
        return;
    }
    if (o.op == VIT_AUG_SOLARIZE) {
        const uint8_t v = (uint8_t)(t < o.iarg ? t : 255 - t);
        lut[t] = lut[256 + t] = lut[512 + t] = v;
        return;
    }
    const bool convex = o.farg >= 0.f && o.farg <= 1.f;
    if (o.op == VIT_AUG_BRIGHTNESS) {
        const uint8_t v = blend_u8(0.f, (float)t, o.farg, convex);
        lut[t] = lut[256 + t] = lut[512 + t] = v;
        return;
    }
    const size_t n = (size_t)npix * 3;
    const uint8_t* src = (o.src ? alt : images) + (size_t)b * n;
    if (o.op == VIT_AUG_CONTRAST) {
        __shared__ unsigned long long lsum;
        if (t == 0) lsum = 0;
        __syncthreads();
        unsigned long long s = 0;
        for (int p = t; p < npix; p += T) s += (unsigned)luma(src[3 * (size_t)p], src[3 * (size_t)p + 1], src[3 * (size_t)p + 2]);
        atomicAdd(&lsum, s);
        __syncthreads();
        // (int)(sum / npix + 0.5) of the double statement: sum / npix is at least 1 / (2 npix) away
        // from any k + 0.5 it does not equal, far more than a double's rounding, so integers give it
        const int m = (int)((2 * lsum + (unsigned long long)npix) / (2 * (unsigned long long)npix));
        const uint8_t v = blend_u8((float)m, (float)t, o.farg, convex);
        lut[t] = lut[256 + t] = lut[512 + t] = v;
        return;
    }
    // AUTOCONTRAST, EQUALIZE: the three histograms, one private copy per wave
    __shared__ unsigned hist[T / 64][768];
    __shared__ double ac_scale[3];
    __shared__ int ac_lo[3];
    for (int i = t; i < (T / 64) * 768; i += T) (&hist[0][0])[i] = 0;
    __syncthreads();
    unsigned* h = hist[t >> 6];
    const int head = chunk_head(src);
    const int nchunks = (int)((head + n + 15) / 16);
    for (int k = t; k < nchunks; k += T) {
        const long long off = (long long)k * 16 - head;
        if (off >= 0 && off + 16 <= (long long)n) {
            const uint4 v = *reinterpret_cast<const uint4*>(src + off);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            int c = (int)(off % 3);
#pragma unroll
            for (int j = 0; j < 16; j++) {
                atomicAdd(&h[c * 256 + ((w[j >> 2] >> (8 * (j & 3))) & 0xffu)], 1u);
                c = c == 2 ? 0 : c + 1;
            }
        } else {
            for (int j = 0; j < 16; j++) {
                const long long q = off + j;
                if (q >= 0 && q < (long long)n) atomicAdd(&h[(int)(q % 3) * 256 + src[q]], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = t; i < 768; i += T) hist[0][i] += hist[1][i] + hist[2][i] + hist[3][i];
    __syncthreads();
    const unsigned* H = hist[0];
    if (o.op == VIT_AUG_AUTOCONTRAST) {
        if (t < 3) {
            int lo = 0, hi = 255;
            while (lo < 255 && H[t * 256 + lo] == 0) lo++;
            while (hi > 0 && H[t * 256 + hi] == 0) hi--;
            ac_lo[t] = lo;
            ac_scale[t] = hi <= lo ? 0.0 : 255.0 / (double)(hi - lo);
        }
        __syncthreads();
        for (int c = 0; c < 3; c++) {
            const double s = ac_scale[c];
            int v = t;
            if (s != 0.0) {
                v = (int)((double)t * s - (double)ac_lo[c] * s);
                v = v < 0 ? 0 : (v > 255 ? 255 : v);
            }
            lut[c * 256 + t] = (uint8_t)v;
        }
        return;
    }
    // EQUALIZE: a serial prefix sum per channel (256 steps, three lanes)
    if (t < 3) {
        const unsigned* hc = H + t * 256;
        int bins = 0, last = 0;
        unsigned total = 0;
        for (int i = 0; i < 256; i++) {
            total += hc[i];
            if (hc[i]) {
                bins++;
                last = i;
            }
        }
        const unsigned step = bins < 2 ? 0u : (total - hc[last]) / 255u;
        unsigned acc = step / 2;
        for (int i = 0; i < 256; i++) {
            unsigned v = (unsigned)i;
            if (step) {
                v = acc / step;
                v = v > 255u ? 255u : v;
                acc += hc[i];
            }
            lut[t * 256 + i] = (uint8_t)v;
        }
    }
}

// ------------------------------------------------------------------------------ in place
__global__ __launch_bounds__(T) void aug_inplace_k(uint8_t* __restrict__ images, uint8_t* __restrict__ alt,
                                                    const DevOp* __restrict__ ops, int stride, int slot, int npix,
                                                    const uint8_t* __restrict__ luts) {
    const int b = blockIdx.y, t = threadIdx.x;
    const DevOp o = ops[(size_t)b * stride + slot];
    const size_t n = (size_t)npix * 3;
    uint8_t* img = (o.src ? alt : images) + (size_t)b * n;
    const long long g = (long long)blockIdx.x * T + t;  // this lane's chunk / pixel group
    if (is_lut_op(o.op)) {
        __shared__ uint8_t lut[768];
        if ((long long)blockIdx.x * T >= max_chunks((int)n)) return;
        for (int i = t; i < 768 / 4; i += T)
            reinterpret_cast<uint32_t*>(lut)[i] = reinterpret_cast<const uint32_t*>(luts + (size_t)b * 768)[i];
        __syncthreads();
        const long long off = g * 16 - chunk_head(img);
        if (off >= (long long)n || off + 16 <= 0) return;
        if (off >= 0 && off + 16 <= (long long)n) {
            uint4 v = *reinterpret_cast<uint4*>(img + off);
            uint32_t w[4] = {v.x, v.y, v.z, v.w};
            int c = (int)(off % 3);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                uint32_t r = 0;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    r |= (uint32_t)lut[c * 256 + ((w[j] >> (8 * i)) & 0xffu)] << (8 * i);
                    c = c == 2 ? 0 : c + 1;
                }
                w[j] = r;
            }
            *reinterpret_cast<uint4*>(img + off) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
            for (int j = 0; j < 16; j++) {
                const long long q = off + j;
                if (q >= 0 && q < (long long)n) img[q] = lut[(int)(q % 3) * 256 + img[q]];
            }
        }
        return;
    }
    if (o.op == VIT_AUG_COLOR) {  // 16 pixels = 48 bytes per lane
        const long long p0 = g * 16;
        if (p0 >= npix) return;
        const bool convex = o.farg >= 0.f && o.farg <= 1.f;
        uint8_t* p = img + p0 * 3;
        if (p0 + 16 <= npix && ((uintptr_t)p & 15) == 0) {
            uint4 v[3] = {reinterpret_cast<uint4*>(p)[0], reinterpret_cast<uint4*>(p)[1], reinterpret_cast<uint4*>(p)[2]};
            uint8_t* bytes = reinterpret_cast<uint8_t*>(v);
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const float l = (float)luma(bytes[3 * i], bytes[3 * i + 1], bytes[3 * i + 2]);
#pragma unroll
                for (int c = 0; c < 3; c++) bytes[3 * i + c] = blend_u8(l, (float)bytes[3 * i + c], o.farg, convex);
            }
            reinterpret_cast<uint4*>(p)[0] = v[0];
            reinterpret_cast<uint4*>(p)[1] = v[1];
            reinterpret_cast<uint4*>(p)[2] = v[2];
        } else {
            const int cnt = (int)(npix - p0 < 16 ? npix - p0 : 16);
            for (int i = 0; i < cnt; i++) {
                const float l = (float)luma(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
                for (int c = 0; c < 3; c++) p[3 * i + c] = blend_u8(l, (float)p[3 * i + c], o.farg, convex);
            }
        }
        return;
    }
    if (o.op == OP_COPY_BACK) {  // the image ended in the scratch buffer
        const uint8_t* from = alt + (size_t)b * n;
        uint8_t* to = images + (size_t)b * n;
        const long long off = g * 16 - chunk_head(to);
        if (off >= (long long)n || off + 16 <= 0) return;
        if (off >= 0 && off + 16 <= (long long)n && ((uintptr_t)(from + off) & 15) == 0) {
            *reinterpret_cast<uint4*>(to + off) = *reinterpret_cast<const uint4*>(from + off);
        } else {
            for (int j = 0; j < 16; j++) {
                const long long q = off + j;
                if (q >= 0 && q < (long long)n) to[q] = from[q];
            }
        }
    }
}

// ------------------------------------------------------------------------------ out of place
__global__ __launch_bounds__(T) void aug_outplace_k(uint8_t* __restrict__ images, uint8_t* __restrict__ alt,
                                                     const DevOp* __restrict__ ops, int stride, int slot, int W,
                                                     uint32_t fill, float k1, float k5) {
    const int b = blockIdx.y;
    const DevOp o = ops[(size_t)b * stride + slot];
    if (o.op < VIT_AUG_SHARPNESS || o.op > VIT_AUG_ROTATE) return;  // uniform over the workgroup
    const int npix = W * W;
    const int p = blockIdx.x * T + threadIdx.x;
    if (p >= npix) return;
    const size_t n = (size_t)npix * 3;
    const uint8_t* src = (o.src ? alt : images) + (size_t)b * n;
    uint8_t* dst = (o.src ? images : alt) + (size_t)b * n;
    const int y = p / W, x = p - y * W;
    uint8_t* out = dst + (size_t)p * 3;
    if (o.op == VIT_AUG_SHARPNESS) {
        const uint8_t* q = src + (size_t)p * 3;
        if (x == 0 || y == 0 || x == W - 1 || y == W - 1) {  // the border keeps its value (blend of v with v)
            out[0] = q[0]; out[1] = q[1]; out[2] = q[2];
            return;
        }
        const bool convex = o.farg >= 0.f && o.farg <= 1.f;
        const int rs = W * 3;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const uint8_t* r1 = q + rs + c;  // ImageFilter.SMOOTH: 0.5, then the rows y+1, y, y-1
            const uint8_t* r0 = q + c;
            const uint8_t* r_1 = q - rs + c;
            float s = 0.5f;
            s = s + (((float)r1[-3] * k1 + (float)r1[0] * k1) + (float)r1[3] * k1);
            s = s + (((float)r0[-3] * k1 + (float)r0[0] * k5) + (float)r0[3] * k1);
            s = s + (((float)r_1[-3] * k1 + (float)r_1[0] * k1) + (float)r_1[3] * k1);
            const float sm = (float)(int)fminf(fmaxf(s, 0.f), 255.f);
            out[c] = blend_u8(sm, (float)r0[0], o.farg, convex);
        }
        return;
    }
    // affine, Pillow's 16.16 fixed point; unsigned arithmetic: the validated end value fits an int
    const int xi = (int)((uint32_t)o.fx[2] + (uint32_t)o.fx[1] * (uint32_t)y + (uint32_t)o.fx[0] * (uint32_t)x) >> 16;
    const int yi = (int)((uint32_t)o.fx[5] + (uint32_t)o.fx[4] * (uint32_t)y + (uint32_t)o.fx[3] * (uint32_t)x) >> 16;
    if (xi >= 0 && xi < W && yi >= 0 && yi < W) {
        const uint8_t* q = src + ((size_t)yi * W + xi) * 3;
        out[0] = q[0]; out[1] = q[1]; out[2] = q[2];
    } else {
        out[0] = (uint8_t)fill; out[1] = (uint8_t)(fill >> 8); out[2] = (uint8_t)(fill >> 16);
    }
}

// ------------------------------------------------------------------------------ host
static bool fix16(double v, int* out) {
    const double r = std::floor(v * 65536.0 + 0.5);
    if (!(std::fabs(r) < 2147483648.0)) return false;
    *out = (int)(long long)r;
    return true;
}

bool prepare(const vit_aug_op_t* plan, int batch, int img, int depth, const unsigned char* fill3, const char* who,
             Prepared& out) {
    if (!plan || !fill3 || batch <= 0 || img <= 0 || img > MAX_IMG) {
        set_error("%s: bad arguments (plan %p, fill %p, batch %d, img %d)", who, (const void*)plan, (const void*)fill3,
                  batch, img);
        return false;
    }
    if (depth < 1 || depth > VIT_AUG_MAX_DEPTH) {
        set_error("%s: depth %d outside 1..%d", who, depth, VIT_AUG_MAX_DEPTH);
        return false;
    }
    out.batch = batch;
    out.img = img;
    out.depth = depth;
    memcpy(out.fill, fill3, 3);
    const int stride = depth + 1;
    out.ops.assign((size_t)batch * stride, DevOp{});
    for (int s = 0; s <= VIT_AUG_MAX_DEPTH; s++) out.lut[s] = out.inplace[s] = out.outplace[s] = false;
    for (int b = 0; b < batch; b++) {
        int cur = 0;
        for (int s = 0; s < depth; s++) {
            const vit_aug_op_t& h = plan[(size_t)b * depth + s];
            DevOp& d = out.ops[(size_t)b * stride + s];
            d.op = h.op;
            d.iarg = h.iarg;
            d.farg = h.farg;
            d.src = cur;
            switch (h.op) {
            case VIT_AUG_IDENTITY:
                break;
            case VIT_AUG_AUTOCONTRAST:
            case VIT_AUG_EQUALIZE:
                out.lut[s] = out.inplace[s] = true;
                break;
            case VIT_AUG_POSTERIZE:
                if (h.iarg < 1 || h.iarg > 8) {
                    set_error("%s: image %d slot %d: posterize bits %d outside 1..8", who, b, s, h.iarg);
                    return false;
                }
                out.lut[s] = out.inplace[s] = true;
                break;
            case VIT_AUG_SOLARIZE:
                if (h.iarg < 0 || h.iarg > 256) {
                    set_error("%s: image %d slot %d: solarize threshold %d outside 0..256", who, b, s, h.iarg);
                    return false;
                }
                out.lut[s] = out.inplace[s] = true;
                break;
            case VIT_AUG_BRIGHTNESS:
            case VIT_AUG_CONTRAST:
            case VIT_AUG_COLOR:
            case VIT_AUG_SHARPNESS:
                if (!(std::isfinite(h.farg) && h.farg >= 0.f)) {
                    set_error("%s: image %d slot %d: factor %g is negative or not finite", who, b, s, (double)h.farg);
                    return false;
                }
                if (h.op == VIT_AUG_SHARPNESS) {
                    out.outplace[s] = true;
                    cur ^= 1;
                } else {
                    out.lut[s] = out.lut[s] || h.op != VIT_AUG_COLOR;
                    out.inplace[s] = true;
                }
                break;
            case VIT_AUG_SHEAR_X:
            case VIT_AUG_SHEAR_Y:
            case VIT_AUG_TRANSLATE_X:
            case VIT_AUG_TRANSLATE_Y:
            case VIT_AUG_ROTATE: {
                const double* a = h.coef;
                bool ok = true;
                for (int i = 0; i < 6; i++) ok = ok && std::isfinite(a[i]);
                if (!ok) {
                    set_error("%s: image %d slot %d: affine coefficient not finite", who, b, s);
                    return false;
                }
                // Pillow's own condition for its fixed-point path: the source coordinates of the four
                // corners stay below 32768 pixels
                const double xs[2] = {0.0, (double)img};
                for (int i = 0; i < 2; i++)
                    for (int j = 0; j < 2; j++)
                        ok = ok && std::fabs(xs[i] * a[0] + xs[j] * a[1] + a[2]) < 32768.0 &&
                             std::fabs(xs[i] * a[3] + xs[j] * a[4] + a[5]) < 32768.0;
                ok = ok && fix16(a[0], &d.fx[0]) && fix16(a[1], &d.fx[1]) && fix16(a[2] + a[0] * 0.5 + a[1] * 0.5, &d.fx[2]) &&
                     fix16(a[3], &d.fx[3]) && fix16(a[4], &d.fx[4]) && fix16(a[5] + a[3] * 0.5 + a[4] * 0.5, &d.fx[5]);
                if (!ok) {
                    set_error("%s: image %d slot %d: affine coefficients leave the 16.16 fixed-point range", who, b, s);
                    return false;
                }
                out.outplace[s] = true;
                cur ^= 1;
                break;
            }
            default:
                set_error("%s: image %d slot %d: unknown op %d", who, b, s, h.op);
                return false;
            }
        }
        DevOp& last = out.ops[(size_t)b * stride + depth];
        last.op = cur ? OP_COPY_BACK : VIT_AUG_IDENTITY;
        last.src = cur;
        if (cur) out.inplace[depth] = true;
    }
    return true;
}

static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
static size_t ops_bytes(int batch) { return align256((size_t)batch * (VIT_AUG_MAX_DEPTH + 1) * sizeof(DevOp)); }
static size_t lut_bytes(int batch) { return align256((size_t)batch * 768); }

size_t scratch_bytes(int batch, int img) {
    return ops_bytes(batch) + lut_bytes(batch) + align256((size_t)batch * img * img * 3);
}

bool enqueue(const Prepared& p, uint8_t* images, void* scratch, hipStream_t st, hipEvent_t read) {
    if (!images || !scratch) {
        set_error("augment: null device buffer");
        return false;
    }
    char* base = (char*)scratch;
    DevOp* dops = (DevOp*)base;
    uint8_t* luts = (uint8_t*)(base + ops_bytes(p.batch));
    uint8_t* alt = luts + lut_bytes(p.batch);
    const int stride = p.depth + 1, npix = p.img * p.img, n = npix * 3;
    bool any = false;
    for (int s = 0; s <= p.depth; s++) any = any || p.inplace[s] || p.outplace[s];
    if (!any) return true;  // identities only
    if (hipMemcpyAsync(dops, p.ops.data(), p.ops.size() * sizeof(DevOp), hipMemcpyHostToDevice, st) != hipSuccess) {
        set_error("augment: plan upload failed");
        return false;
    }
    if (read) VIT_HIP(hipEventRecord(read, st));
    const uint32_t fill = (uint32_t)p.fill[0] | (uint32_t)p.fill[1] << 8 | (uint32_t)p.fill[2] << 16;
    const dim3 grid_in((unsigned)((max_chunks(n) + T - 1) / T), (unsigned)p.batch);
    const dim3 grid_out((unsigned)((npix + T - 1) / T), (unsigned)p.batch);
    for (int s = 0; s <= p.depth; s++) {
        if (p.lut[s]) {
            aug_lut_k<<<p.batch, T, 0, st>>>(images, alt, dops, stride, s, npix, luts);
            count_hit(VIT_HIT_AUGMENT + 0);
        }
        if (p.inplace[s]) {
            aug_inplace_k<<<grid_in, T, 0, st>>>(images, alt, dops, stride, s, npix, luts);
            count_hit(VIT_HIT_AUGMENT + (s == p.depth ? 3 : 1));
        }
        if (p.outplace[s]) {
            aug_outplace_k<<<grid_out, T, 0, st>>>(images, alt, dops, stride, s, p.img, fill, 1.f / 13.f, 5.f / 13.f);
            count_hit(VIT_HIT_AUGMENT + 2);
        }
    }
    if (hipGetLastError() != hipSuccess) {
        set_error("augment: kernel launch failed");
        return false;
    }
    return true;
}

// the generator of the loaders' shuffle and crop draws (loader.hip, jpeg.hip)
static uint64_t sm64(uint64_t seed, uint64_t i) {
    uint64_t z = seed + (i + 1) * 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

}  // namespace aug
}  // namespace vit

using vit::set_error;
using namespace vit::aug;

extern "C" {

int vit_randaugment_draw(unsigned long long seed, long long key, int num_ops, int magnitude, int img,
                         vit_aug_op_t* out) {
    if (!out || num_ops < 1 || num_ops > VIT_AUG_MAX_DEPTH || magnitude < 0 || magnitude > 30 || img <= 0 ||
        img > MAX_IMG) {
        set_error("vit_randaugment_draw: bad arguments (num_ops %d of 1..%d, magnitude %d of 0..30, img %d)", num_ops,
                  VIT_AUG_MAX_DEPTH, magnitude, img);
        return 1;
    }
    const uint64_t s = (uint64_t)seed ^ sm64(0x72616e64617567ULL, (uint64_t)key);
    const int m = magnitude;
    for (int j = 0; j < num_ops; j++) {
        vit_aug_op_t& o = out[j];
        memset(&o, 0, sizeof(o));
        o.op = (int)(sm64(s, 2 * (uint64_t)j) % VIT_AUG_NUM_OPS);
        const double sg = (sm64(s, 2 * (uint64_t)j + 1) & 1) ? -1.0 : 1.0;
        o.farg = 1.f;
        o.coef[0] = 1.0;
        o.coef[4] = 1.0;
        switch (o.op) {
        case VIT_AUG_SHEAR_X:
            o.coef[1] = sg * (0.3 * m / 30.0);
            break;
        case VIT_AUG_SHEAR_Y:
            o.coef[3] = sg * (0.3 * m / 30.0);
            break;
        case VIT_AUG_TRANSLATE_X:
            o.coef[2] = sg * (double)(int)((150.0 / 331.0) * img * m / 30.0);
            break;
        case VIT_AUG_TRANSLATE_Y:
            o.coef[5] = sg * (double)(int)((150.0 / 331.0) * img * m / 30.0);
            break;
        case VIT_AUG_ROTATE: {
            const double deg = sg * (30.0 * m / 30.0);
            const double th = -deg * 3.141592653589793 / 180.0;
            const double a = std::cos(th), b = std::sin(th), d = -std::sin(th), e = a;
            const double cx = img / 2.0, cy = img / 2.0;
            o.coef[0] = a; o.coef[1] = b; o.coef[2] = cx - (a * cx + b * cy);
            o.coef[3] = d; o.coef[4] = e; o.coef[5] = cy - (d * cx + e * cy);
            break;
        }
        case VIT_AUG_BRIGHTNESS:
        case VIT_AUG_CONTRAST:
        case VIT_AUG_COLOR:
        case VIT_AUG_SHARPNESS:
            o.farg = (float)(1.0 + sg * (0.9 * m / 30.0));
            break;
        case VIT_AUG_POSTERIZE:
            o.iarg = 8 - (int)(m / 7.5);
            break;
        case VIT_AUG_SOLARIZE:
            o.iarg = (int)std::ceil(255.0 * (1.0 - m / 30.0));
            break;
        default:
            break;
        }
    }
    return 0;
}

int vit_augment_u8(unsigned char* dev_images, int batch, int img, const vit_aug_op_t* host_plan, int depth,
                   const unsigned char* fill3, void* stream) {
    if (!dev_images) {
        set_error("vit_augment_u8: null images");
        return 1;
    }
    Prepared p;
    if (!prepare(host_plan, batch, img, depth, fill3, "vit_augment_u8", p)) return 1;
    // this entry point's own scratch, per host thread (the stream is the caller's choice, so the
    // context workspace, which follows the context stream, does not serve)
    struct Scratch {
        void* p = nullptr;
        size_t bytes = 0;
        hipEvent_t read = nullptr;
    };
    static thread_local Scratch sc;
    const size_t need = scratch_bytes(batch, img);
    if (need > sc.bytes) {
        if (sc.p) (void)hipFree(sc.p);  // waits for the device
        sc.p = nullptr;
        sc.bytes = 0;
        if (hipMalloc(&sc.p, need) != hipSuccess) {
            sc.p = nullptr;
            set_error("vit_augment_u8: hipMalloc(%zu) failed", need);
            return 1;
        }
        sc.bytes = need;
    }
    if (!sc.read && hipEventCreateWithFlags(&sc.read, hipEventDisableTiming) != hipSuccess) {
        set_error("vit_augment_u8: event creation failed");
        return 1;
    }
    hipStream_t st = stream ? (hipStream_t)stream : vit::stream();
    // p.ops is read by the upload: wait for it (not for the kernels) before p goes away; an
    // identities-only plan uploads nothing and leaves the event as it was
    const bool ok = enqueue(p, dev_images, sc.p, st, sc.read);
    VIT_HIP(hipEventSynchronize(sc.read));
    return ok && !vit::has_error() ? 0 : 1;
}

}  // extern "C"
