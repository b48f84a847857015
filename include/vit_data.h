/*
 * vit_data.h — input pipeline of libvit_hip.so.
 *
 * The reference's forward takes an already-built input array (ViT::forward(inputs, targets, B, T),
 * /root/reference/train_vit.rs:188; encoder_forward :196) and has no data loader.  This is the
 * MI355X-side feed for real images:
 *
 *   vit_loader_*   native record loader: a raw uint8 image file [N, img, img, 3] (HWC, RGB) and a
 *                  raw int32 label file [N], memory-mapped; a per-epoch seeded shuffle; the batch
 *                  of each data-parallel rank; batches assembled by a background thread into a
 *                  ring of (pinned) host buffers.
 *   vit_trainer_set_batch_u8
 *                  copies one uint8 batch to the device on a copy stream (double-buffered device
 *                  staging, overlapping the previous step's kernels) and normalises it on the
 *                  device into the trainer's fp32 [B, 3, img, img] pixels:
 *                      pixel[b][c][y][x] = (u8[b][y][x][c] / 255 - mean[c]) / std[c]
 *                  (fp32, each operation correctly rounded, in that order).
 *
 * Shuffle: epoch e uses the permutation of Fisher-Yates (i = N-1 .. 1, swap(i, r_i mod (i+1)))
 * with r_i = splitmix64 counter stream of seed + e at position N-1-i (the generator of the
 * package's synthetic data, vit.rs_amd/data.py); shuffle = 0 keeps file order.  Step k of an
 * epoch gives rank r the records perm[(k*world + r)*batch .. +batch); the last partial global
 * batch is dropped, so every rank sees the same number of steps and disjoint records.
 */
#ifndef VIT_DATA_H
#define VIT_DATA_H

#include "vit_trainer.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vit_loader vit_loader_t;

/* pinned = 1: ring buffers in page-locked memory (hipHostMalloc; asynchronous DMA);
 * 0: malloc (no HIP call at all — usable without a GPU).  depth = ring slots (>= 2).
 * Returns NULL on error (vit_last_error). */
vit_loader_t* vit_loader_open(const char* images_path, const char* labels_path, int img,
                              int batch, unsigned long long seed, int rank, int world, int shuffle,
                              int pinned, int depth);
long long vit_loader_num_records(const vit_loader_t* l);
int vit_loader_steps_per_epoch(const vit_loader_t* l);
/* Blocks until the next batch is assembled.  images -> [batch, img, img, 3] uint8, labels ->
 * [batch] int32, valid until the next vit_loader_next / vit_loader_close.  epoch / step
 * (nullable) identify the batch.  Returns 0, or non-zero on error. */
int vit_loader_next(vit_loader_t* l, const unsigned char** images, const int** labels,
                    long long* epoch, int* step);
void vit_loader_close(vit_loader_t* l);

/* host pointers; labels NULL = forward-only batch.  Returns once the host buffers have been read
 * (they may be reused immediately); the device work is ordered before the next forward. */
int vit_trainer_set_batch_u8(vit_trainer_t* t, const unsigned char* images, const int* labels,
                             const float* mean3, const float* std3);

/* ---- RandAugment on the device uint8 batch.
 *
 * The 14 ops of the torchvision RandAugment space on one RGB uint8 image (HWC); each equals the
 * Pillow call named, byte for byte (vit.rs_amd/augment.py reference_apply is the numpy statement):
 *   IDENTITY
 *   AUTOCONTRAST  ImageOps.autocontrast: per channel lo / hi = min / max; hi <= lo keeps the
 *                 channel; else lut[i] = clip((int)(i * s - lo * s), 0, 255), s = 255.0 / (hi - lo)
 *                 (double, product and difference each rounded).
 *   EQUALIZE      ImageOps.equalize: per channel h = histogram; fewer than 2 non-empty bins keeps
 *                 the channel; step = (sum(h) - last non-empty bin) / 255 (integer), 0 keeps it;
 *                 else n = step / 2, for i = 0..255: lut[i] = min(n / step, 255), n += h[i].
 *   POSTERIZE     iarg = bits 1..8: v & ~(2^(8-bits) - 1).
 *   SOLARIZE      iarg = threshold 0..256: v < thr ? v : 255 - v.
 *   BRIGHTNESS    farg = f >= 0: blend(0, v, f).
 *   CONTRAST      blend(m, v, f), m = (int)(mean(L) + 0.5) over the image.
 *   COLOR         blend(L, v, f) per pixel.
 *   SHARPNESS     blend(S, v, f), S = ImageFilter.SMOOTH: 3x3 taps (1,1,1,1,5,1,1,1,1), each
 *                 (float)w / 13.f; t = 0.5f, then t += (p[x-1] k0 + p[x] k1) + p[x+1] k2 for the rows
 *                 y+1, y, y-1 in that order (fp32, every operation rounded), clipped to [0, 255],
 *                 truncated; the one-pixel border keeps its value.
 *   SHEAR_X .. ROTATE   coef = (a, b, c, d, e, f) of Image.transform(size, AFFINE, coef, NEAREST,
 *                 fillcolor): FIX(v) = floor(v * 65536 + 0.5); output (x, y) reads input
 *                 xi = (FIX(c + a/2 + b/2) + FIX(b) y + FIX(a) x) >> 16, yi likewise from d, e, f
 *                 (arithmetic shift); outside the image gives the fill colour.
 *   L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16.
 *   blend(d, v, f): t = (float)d + f * ((float)v - (float)d), fp32, no fused multiply-add;
 *   (uint8)(int)t for 0 <= f <= 1, else t clipped to [0, 255] first. */
enum {
    VIT_AUG_IDENTITY = 0,
    VIT_AUG_AUTOCONTRAST = 1,
    VIT_AUG_EQUALIZE = 2,
    VIT_AUG_POSTERIZE = 3,
    VIT_AUG_SOLARIZE = 4,
    VIT_AUG_BRIGHTNESS = 5,
    VIT_AUG_CONTRAST = 6,
    VIT_AUG_COLOR = 7,
    VIT_AUG_SHARPNESS = 8,
    VIT_AUG_SHEAR_X = 9,
    VIT_AUG_SHEAR_Y = 10,
    VIT_AUG_TRANSLATE_X = 11,
    VIT_AUG_TRANSLATE_Y = 12,
    VIT_AUG_ROTATE = 13,
    VIT_AUG_NUM_OPS = 14,
    VIT_AUG_MAX_DEPTH = 4
};
typedef struct {
    int op;         /* VIT_AUG_* */
    int iarg;       /* POSTERIZE bits, SOLARIZE threshold */
    float farg;     /* the four enhancers' factor */
    int reserved;   /* 0 */
    double coef[6]; /* the affine ops' (a, b, c, d, e, f) */
} vit_aug_op_t;

/* Applies host_plan [batch][depth] (slot 0 first) to dev_images [batch][img][img][3] uint8 (device),
 * in place, on stream (a hipStream_t; NULL = the context stream); fill3 = the affine ops' fill
 * colour.  The whole plan is validated before any GPU work: an unknown op, bits outside 1..8, a
 * threshold outside 0..256, a negative or non-finite factor, a non-finite coefficient or one whose
 * source coordinates leave the 16.16 range (|.| >= 32768 pixels at an image corner), or depth
 * outside 1..VIT_AUG_MAX_DEPTH returns non-zero with vit_last_error and leaves the images
 * untouched.  Returns once the host plan has been read. */
int vit_augment_u8(unsigned char* dev_images, int batch, int img, const vit_aug_op_t* host_plan, int depth,
                   const unsigned char* fill3, void* stream);

/* Host only (no HIP call): the RandAugment policy draw of one image -> out[num_ops].
 * num_ops 1..VIT_AUG_MAX_DEPTH, magnitude m = 0..30 (31 bins).  Random words: w_k =
 * splitmix64 counter stream of s = seed ^ splitmix64(0x72616e64617567, key) at position k (the
 * generator of the loaders' shuffle; the crop draw uses another tag).  Slot j takes two words:
 * op = w_2j mod 14 (the VIT_AUG_* value), negative = w_(2j+1) & 1 (drawn for every op, used by the
 * signed ones).  With sg = negative ? -1 : 1:
 *   SHEAR_X      v = sg 0.3 m / 30, coef (1, v, 0, 0, 1, 0);   SHEAR_Y  coef (1, 0, 0, v, 1, 0)
 *   TRANSLATE_X  p = sg (int)((150.0 / 331.0) img m / 30), coef (1, 0, p, 0, 1, 0);
 *   TRANSLATE_Y  coef (1, 0, 0, 0, 1, p)
 *   ROTATE       th = -(sg 30 m / 30) pi / 180; a = e = cos th, b = sin th, d = -sin th,
 *                c = cx - (a cx + b cy), f = cy - (d cx + e cy), cx = cy = img / 2.0
 *   BRIGHTNESS, CONTRAST, COLOR, SHARPNESS   farg = (float)(1 + sg 0.9 m / 30)
 *   POSTERIZE    iarg = 8 - (int)(m / 7.5);   SOLARIZE  iarg = ceil(255 (1 - m / 30.0))
 * (all in double, evaluated left to right as written; x m / 30 means x * m / 30.0).  Other ops
 * carry coef (1, 0, 0, 0, 1, 0), iarg 0 and farg 1. */
int vit_randaugment_draw(unsigned long long seed, long long key, int num_ops, int magnitude, int img,
                         vit_aug_op_t* out);

/* One-shot: host_plan [batch][depth] is applied to the next vit_trainer_set_batch_u8 only, on the
 * copy stream between the upload and the normalise.  NULL clears a pending plan.  An invalid plan
 * (as vit_augment_u8) is rejected here. */
int vit_trainer_set_augment_plan(vit_trainer_t* t, const vit_aug_op_t* host_plan, int depth,
                                 const unsigned char* fill3);

#ifdef __cplusplus
}
#endif
#endif
