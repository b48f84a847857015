"""Random erasing (timm's RandomErasing) on the normalised fp32 batch: the per-image draw of the boxes
and the numpy statement of what vit_random_erase_f32 / vit_trainer_erase_batch write.

draw() wraps the library's host-only vit_random_erase_draw; reference_draw() is its Python statement
(the math module's exp / log / sqrt: the platform libm the C side calls, not numpy's vector forms);
reference_apply() is the float64 statement of the kernel; Eraser draws a batch's boxes from its keys.
Host-only: nothing here touches the GPU.
"""
import ctypes
import math

import numpy as np

ERASE_CONST, ERASE_RAND, ERASE_PIXEL = 0, 1, 2  # include/vit_ops.h VIT_ERASE_*
DRAW_TAG = 0x6572617365  # "erase"
NOISE_TAG = 0x65726E6F697365  # "ernoise"
ATTEMPTS = 10
MAX_COUNT = 4
# timm's defaults
MIN_AREA, MAX_AREA, MIN_ASPECT, MAX_ASPECT = 0.02, 1.0 / 3.0, 0.3, 1.0 / 0.3
_M = (1 << 64) - 1


def splitmix64(seed, i):
    z = (seed + (i + 1) * 0x9E3779B97F4A7C15) & _M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M
    return z ^ (z >> 31)


def _check_draw_args(img, prob, min_area, max_area, min_aspect, max_aspect, min_count, max_count):
    if img < 1:
        raise ValueError("img < 1")
    if not 0.0 <= prob <= 1.0:
        raise ValueError("prob outside [0, 1]")
    if not 0.0 < min_area <= max_area <= 1.0:
        raise ValueError("areas not 0 < min <= max <= 1")
    if not (0.0 < min_aspect <= max_aspect and math.isfinite(max_aspect)):
        raise ValueError("aspects not 0 < min <= max")
    if not 1 <= min_count <= max_count <= MAX_COUNT:
        raise ValueError("counts not 1 <= min <= max <= 4")


def reference_draw(seed, key, img, prob, min_area=MIN_AREA, max_area=MAX_AREA, min_aspect=MIN_ASPECT,
                   max_aspect=MAX_ASPECT, min_count=1, max_count=1):
    """(boxes int32 [max_count, 4] = x0, y0, x1, y1, count) as vit_random_erase_draw computes them, exactly:
    timm's RandomErasing._erase for one square image on the splitmix64 counter stream of
    s = seed ^ splitmix64("erase", key), u = (w >> 11) * 2^-53."""
    _check_draw_args(img, prob, min_area, max_area, min_aspect, max_aspect, min_count, max_count)
    s = (seed & _M) ^ splitmix64(DRAW_TAG, key & _M)

    def uni(pos):
        return float(splitmix64(s, pos) >> 11) * 2.0 ** -53

    boxes = np.zeros((max_count, 4), np.int32)
    if not uni(0) < prob:
        return boxes, 0
    count = min_count + int(math.floor(uni(1) * float(max_count - min_count + 1)))
    la, lb = math.log(min_aspect), math.log(max_aspect)
    for k in range(count):
        for a in range(ATTEMPTS):
            at = 2 + (k * ATTEMPTS + a) * 4
            target = (min_area + uni(at) * (max_area - min_area)) * (float(img) * float(img)) / float(count)
            aspect = math.exp(la + uni(at + 1) * (lb - la))
            h = int(round(math.sqrt(target * aspect)))  # round(): ties to even, as rint
            w = int(round(math.sqrt(target / aspect)))
            if w < img and h < img:
                top = int(math.floor(uni(at + 2) * float(img - h + 1)))
                left = int(math.floor(uni(at + 3) * float(img - w + 1)))
                boxes[k] = (left, top, left + w, top + h)
                break
    return boxes, count


def draw(seed, key, img, prob, min_area=MIN_AREA, max_area=MAX_AREA, min_aspect=MIN_ASPECT, max_aspect=MAX_ASPECT,
         min_count=1, max_count=1):
    """vit_random_erase_draw: (boxes int32 [max_count, 4], count)."""
    from . import check, lib
    n = max(int(max_count), 1)
    boxes = np.zeros((n, 4), np.int32)
    count = ctypes.c_int(0)
    if lib().vit_random_erase_draw(ctypes.c_ulonglong(seed & _M), int(key), int(img), float(prob), float(min_area),
                                   float(max_area), float(min_aspect), float(max_aspect), int(min_count),
                                   int(max_count), boxes.ctypes.data_as(ctypes.c_void_p), ctypes.byref(count)):
        check("vit_random_erase_draw")
        raise ValueError("vit_random_erase_draw failed")
    return boxes, int(count.value)


def noise_seed(seed, key):
    """sn, the noise stream of the image with this key."""
    return (seed & _M) ^ splitmix64(NOISE_TAG, key & _M)


_C1, _C2, _C3 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def normals(sn, pos):
    """z(p) in float64 (not yet rounded to fp32) for an integer array of positions of the stream sn:
    u1 = ((w >> 40) + 1) 2^-24, u2 = ((w >> 16) & 0xFFFFFF) 2^-24, z = sqrt(-2 log u1) cos(6.283185307179586 u2)."""
    p = np.asarray(pos).astype(np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(sn) + (p + np.uint64(1)) * _C1
        z = (z ^ (z >> np.uint64(30))) * _C2
        z = (z ^ (z >> np.uint64(27))) * _C3
        w = z ^ (z >> np.uint64(31))
    u1 = ((w >> np.uint64(40)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = ((w >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


def check_boxes(boxes, B, img):
    """boxes as int32 [B, max_count, 4], validated as the library validates them."""
    bx = np.ascontiguousarray(boxes, dtype=np.int32)
    if bx.ndim != 3 or bx.shape[0] != B or bx.shape[2] != 4 or not 1 <= bx.shape[1] <= MAX_COUNT:
        raise ValueError(f"boxes {bx.shape} not [{B}, 1..4, 4]")
    x0, y0, x1, y1 = (bx[..., i] for i in range(4))
    if ((x0 < 0) | (x0 > x1) | (x1 > img) | (y0 < 0) | (y0 > y1) | (y1 > img)).any():
        raise ValueError("a box is not 0 <= x0 <= x1 <= img, 0 <= y0 <= y1 <= img")
    return bx


def reference_apply(pixels, boxes, mode, seed=0, keys=None):
    """float64 statement of vit_random_erase_f32 on pixels [B, 3, img, img] with boxes [B, max_count, 4]:
    returns float64 [B, 3, img, img]; outside the boxes the input's values (exactly, so .astype(float32)
    gives the input's bits), inside +0.0 (CONST), z(p) at p = (c img + y) img + x (PIXEL) or the box's
    colour z(3 img^2 + 3 k + c) (RAND; where boxes overlap, the later box's).  The device result is this
    rounded to fp32 once."""
    px = np.asarray(pixels)
    B, img = px.shape[0], px.shape[-1]
    assert px.shape == (B, 3, img, img)
    bx = check_boxes(boxes, B, img)
    if mode not in (ERASE_CONST, ERASE_RAND, ERASE_PIXEL):
        raise ValueError(f"unknown erase mode {mode}")
    if mode != ERASE_CONST and keys is None:
        raise ValueError("the noise modes need keys")
    out = px.astype(np.float64)
    pos = np.arange(3 * img * img, dtype=np.int64).reshape(3, img, img)
    for b in range(B):
        sn = noise_seed(seed, int(keys[b])) if mode != ERASE_CONST else 0
        for k in range(bx.shape[1]):
            x0, y0, x1, y1 = (int(v) for v in bx[b, k])
            if x1 == x0 or y1 == y0:
                continue
            if mode == ERASE_CONST:
                out[b, :, y0:y1, x0:x1] = 0.0
            elif mode == ERASE_PIXEL:
                out[b, :, y0:y1, x0:x1] = normals(sn, pos[:, y0:y1, x0:x1])
            else:
                col = normals(sn, 3 * img * img + 3 * k + np.arange(3))
                out[b, :, y0:y1, x0:x1] = col[:, None, None]
    return out


def inside_mask(boxes, B, img):
    """bool [B, 1, img, img]: the pixels some box covers."""
    bx = check_boxes(boxes, B, img)
    m = np.zeros((B, 1, img, img), bool)
    for b in range(B):
        for x0, y0, x1, y1 in bx[b]:
            m[b, :, y0:y1, x0:x1] = True
    return m


class Eraser:
    """Random erasing with probability `prob` per image (DeiT: 0.25, ERASE_PIXEL, one box).

    boxes(keys, img) draws each image's boxes from its key -> int32 [B, max_count, 4];
    apply(model, keys) draws them for model's batch and erases it (ViT.erase_batch) with the same keys for
    the noise; call it after set_batch* and before mix_batch.  Keys are the caller's: epoch * N + record
    where the record is known, keys_for_step() otherwise."""

    def __init__(self, prob=0.25, mode=ERASE_PIXEL, min_area=MIN_AREA, max_area=MAX_AREA, min_aspect=MIN_ASPECT,
                 max_aspect=MAX_ASPECT, min_count=1, max_count=None, seed=1337):
        max_count = min_count if max_count is None else max_count
        _check_draw_args(1, prob, min_area, max_area, min_aspect, max_aspect, min_count, max_count)
        if mode not in (ERASE_CONST, ERASE_RAND, ERASE_PIXEL):
            raise ValueError(f"unknown erase mode {mode}")
        self.prob, self.mode, self.seed = float(prob), int(mode), int(seed)
        self.area = (float(min_area), float(max_area))
        self.aspect = (float(min_aspect), float(max_aspect))
        self.counts = (int(min_count), int(max_count))

    @staticmethod
    def keys_for_step(step, batch, rank=0, world=1):
        """(step * world + rank) * batch + i: ranks of a data-parallel job draw different boxes."""
        return (int(step) * int(world) + int(rank)) * int(batch) + np.arange(batch, dtype=np.int64)

    def boxes(self, keys, img):
        keys = np.asarray(keys, dtype=np.int64)
        out = np.zeros((keys.size, self.counts[1], 4), np.int32)
        for i, key in enumerate(keys):
            out[i], _ = draw(self.seed, int(key), img, self.prob, *self.area, *self.aspect, *self.counts)
        return out

    def apply(self, model, keys):
        keys = np.ascontiguousarray(keys, dtype=np.int64)
        bx = self.boxes(keys, model.cfg.img)
        if self.prob > 0.0:
            model.erase_batch(bx, self.mode, self.seed, keys)
        return bx
