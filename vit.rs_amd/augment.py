"""RandAugment on uint8 images: the per-image policy draw (reference_draw, RandAugment) and the numpy
statement of what vit_augment_u8 computes (reference_apply), byte for byte Pillow's result for the
same arguments (include/vit_data.h lists the ops).

A plan is a nested list [batch][depth] of ops (op, iarg, farg, coef): op one of the constants below,
iarg the posterize bits / solarize threshold, farg the enhancers' factor, coef the six affine
coefficients (a, b, c, d, e, f) of Image.transform(size, AFFINE, coef, NEAREST).
Host-only (numpy): nothing here touches the GPU.
"""
import ctypes
import math

import numpy as np

(IDENTITY, AUTOCONTRAST, EQUALIZE, POSTERIZE, SOLARIZE, BRIGHTNESS, CONTRAST, COLOR, SHARPNESS,
 SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y, ROTATE) = range(14)  # include/vit_data.h VIT_AUG_*
NUM_OPS, MAX_DEPTH = 14, 4
OP_NAMES = ("identity", "autocontrast", "equalize", "posterize", "solarize", "brightness", "contrast",
            "color", "sharpness", "shear_x", "shear_y", "translate_x", "translate_y", "rotate")
ENHANCERS = (BRIGHTNESS, CONTRAST, COLOR, SHARPNESS)
AFFINE = (SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y, ROTATE)
UNIT = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
DRAW_TAG = 0x72616e64617567  # "randaug"; the crop draw's tag is 0x6a70656755
_M = (1 << 64) - 1


class AugOp(ctypes.Structure):
    """vit_aug_op_t."""
    _fields_ = [("op", ctypes.c_int), ("iarg", ctypes.c_int), ("farg", ctypes.c_float),
                ("reserved", ctypes.c_int), ("coef", ctypes.c_double * 6)]


def op(kind, iarg=0, farg=1.0, coef=UNIT):
    return (int(kind), int(iarg), float(farg), tuple(float(c) for c in coef))


def plan_to_c(plan):
    """[batch][depth] ops -> (AugOp array of batch * depth, batch, depth)."""
    batch, depth = len(plan), len(plan[0])
    arr = (AugOp * (batch * depth))()
    for b, row in enumerate(plan):
        assert len(row) == depth, "every image takes the same number of ops"
        for s, (kind, iarg, farg, coef) in enumerate(row):
            arr[b * depth + s] = AugOp(kind, iarg, farg, 0, (ctypes.c_double * 6)(*coef))
    return arr, batch, depth


def plan_from_c(arr, batch, depth):
    return [[op(arr[b * depth + s].op, arr[b * depth + s].iarg, arr[b * depth + s].farg,
                tuple(arr[b * depth + s].coef)) for s in range(depth)] for b in range(batch)]


# --------------------------------------------------------------------------- coefficient helpers
def shear_x(v):
    return op(SHEAR_X, coef=(1.0, v, 0.0, 0.0, 1.0, 0.0))


def shear_y(v):
    return op(SHEAR_Y, coef=(1.0, 0.0, 0.0, v, 1.0, 0.0))


def translate_x(p):
    return op(TRANSLATE_X, coef=(1.0, 0.0, p, 0.0, 1.0, 0.0))


def translate_y(p):
    return op(TRANSLATE_Y, coef=(1.0, 0.0, 0.0, 0.0, 1.0, p))


def rotate(deg, img):
    """Rotation by deg degrees (counter-clockwise, as Image.rotate) about the image centre."""
    th = -deg * math.pi / 180.0
    a = math.cos(th)
    b = math.sin(th)
    d = -math.sin(th)
    e = a
    cx = cy = img / 2.0
    return op(ROTATE, coef=(a, b, cx - (a * cx + b * cy), d, e, cy - (d * cx + e * cy)))


# --------------------------------------------------------------------------- the draw
def splitmix64(seed, i):
    z = (seed + (i + 1) * 0x9E3779B97F4A7C15) & _M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M
    return z ^ (z >> 31)


def reference_draw(seed, key, num_ops, magnitude, img):
    """The policy draw of one image, as vit_randaugment_draw: a list of num_ops ops."""
    assert 1 <= num_ops <= MAX_DEPTH and 0 <= magnitude <= 30 and img > 0
    s = (seed & _M) ^ splitmix64(DRAW_TAG, key & _M)
    m = int(magnitude)
    out = []
    for j in range(num_ops):
        kind = splitmix64(s, 2 * j) % NUM_OPS
        sg = -1.0 if splitmix64(s, 2 * j + 1) & 1 else 1.0
        if kind == SHEAR_X:
            out.append(shear_x(sg * (0.3 * m / 30.0)))
        elif kind == SHEAR_Y:
            out.append(shear_y(sg * (0.3 * m / 30.0)))
        elif kind == TRANSLATE_X:
            out.append(translate_x(sg * float(int((150.0 / 331.0) * img * m / 30.0))))
        elif kind == TRANSLATE_Y:
            out.append(translate_y(sg * float(int((150.0 / 331.0) * img * m / 30.0))))
        elif kind == ROTATE:
            out.append(rotate(sg * (30.0 * m / 30.0), img))
        elif kind in ENHANCERS:
            out.append(op(kind, farg=float(np.float32(1.0 + sg * (0.9 * m / 30.0)))))
        elif kind == POSTERIZE:
            out.append(op(kind, iarg=8 - int(m / 7.5)))
        elif kind == SOLARIZE:
            out.append(op(kind, iarg=int(math.ceil(255.0 * (1.0 - m / 30.0)))))
        else:
            out.append(op(kind))
    return out


class RandAugment:
    """The batch plan of RandAugment(num_ops, magnitude): image i of the k-th batch is drawn with
    key = k * batch + i, or with the keys given (e.g. epoch * N + record, as the JPEG loader)."""

    def __init__(self, num_ops=2, magnitude=9, seed=0):
        self.num_ops, self.magnitude, self.seed = int(num_ops), int(magnitude), int(seed)
        self.count = 0

    def plan(self, batch, img, keys=None):
        if keys is None:
            keys = range(self.count, self.count + batch)
            self.count += batch
        return [reference_draw(self.seed, int(k), self.num_ops, self.magnitude, img) for k in keys]


# --------------------------------------------------------------------------- the ops
def _luma(im):
    r, g, b = (im[..., c].astype(np.int64) for c in range(3))
    return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16


def _blend(d, v, f):
    """Image.blend(degenerate d, image v, f): fp32, each operation rounded."""
    f = np.float32(f)
    d = np.asarray(d).astype(np.float32)
    v = np.asarray(v).astype(np.float32)
    t = d + f * (v - d)
    assert t.dtype == np.float32
    if not (f >= 0 and f <= 1):
        t = np.clip(t, np.float32(0), np.float32(255))
    return t.astype(np.int32).astype(np.uint8)


def _autocontrast_lut(ch):
    lo, hi = int(ch.min()), int(ch.max())
    if hi <= lo:
        return np.arange(256, dtype=np.uint8)
    scale = 255.0 / (hi - lo)
    return np.array([min(max(int(i * scale - lo * scale), 0), 255) for i in range(256)], np.uint8)


def _equalize_lut(ch):
    h = np.bincount(ch.ravel(), minlength=256)
    nz = np.nonzero(h)[0]
    ident = np.arange(256, dtype=np.uint8)
    if nz.size < 2:
        return ident
    step = (int(h.sum()) - int(h[nz[-1]])) // 255
    if step == 0:
        return ident
    lut = np.zeros(256, np.uint8)
    n = step // 2
    for i in range(256):
        lut[i] = min(n // step, 255)
        n += int(h[i])
    return lut


_SMOOTH = [np.float32(w) / np.float32(13) for w in (1, 1, 1, 1, 5, 1, 1, 1, 1)]


def _smooth(im):
    """ImageFilter.SMOOTH on HxWx3 uint8."""
    H, W = im.shape[:2]
    out = im.copy()
    if H < 3 or W < 3:
        return out
    p = im.astype(np.float32)
    t = np.full((H - 2, W - 2, 3), np.float32(0.5), np.float32)
    for dy in (2, 1, 0):  # rows y+1, y, y-1; the taps are symmetric
        k = _SMOOTH[3 * dy:3 * dy + 3]
        r = p[dy:dy + H - 2]
        t = t + ((r[:, 0:W - 2] * k[0] + r[:, 1:W - 1] * k[1]) + r[:, 2:W] * k[2])
    assert t.dtype == np.float32
    out[1:-1, 1:-1] = np.clip(t, np.float32(0), np.float32(255)).astype(np.int32).astype(np.uint8)
    return out


def fix16(v):
    return int(math.floor(v * 65536.0 + 0.5))


def _affine(im, coef, fill):
    H, W = im.shape[:2]
    a, b, c, d, e, f = coef
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    xi = (fix16(c + a * 0.5 + b * 0.5) + fix16(b) * y + fix16(a) * x) >> 16
    yi = (fix16(f + d * 0.5 + e * 0.5) + fix16(e) * y + fix16(d) * x) >> 16
    ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
    out = np.empty_like(im)
    out[...] = np.asarray(fill, np.uint8)
    out[ok] = im[yi[ok], xi[ok]]
    return out


def apply_op(im, o, fill=(0, 0, 0)):
    """One op on one HxWx3 uint8 image -> a new image."""
    kind, iarg, farg, coef = o
    if kind == IDENTITY:
        return im.copy()
    if kind == AUTOCONTRAST:
        return np.stack([_autocontrast_lut(im[..., c])[im[..., c]] for c in range(3)], -1)
    if kind == EQUALIZE:
        return np.stack([_equalize_lut(im[..., c])[im[..., c]] for c in range(3)], -1)
    if kind == POSTERIZE:
        assert 1 <= iarg <= 8
        return im & np.uint8(~((1 << (8 - iarg)) - 1) & 0xFF)
    if kind == SOLARIZE:
        assert 0 <= iarg <= 256
        return np.where(im.astype(np.int32) < iarg, im, 255 - im).astype(np.uint8)
    if kind == BRIGHTNESS:
        return _blend(np.zeros_like(im), im, farg)
    if kind == CONTRAST:
        L = _luma(im)
        m = int(float(int(L.sum())) / float(L.size) + 0.5)
        return _blend(np.full_like(im, m), im, farg)
    if kind == COLOR:
        return _blend(np.repeat(_luma(im)[..., None], 3, -1), im, farg)
    if kind == SHARPNESS:
        return _blend(_smooth(im), im, farg)
    if kind in AFFINE:
        return _affine(im, coef, fill)
    raise ValueError(f"unknown augment op {kind}")


def reference_apply(images_u8, plan, fill=(0, 0, 0)):
    """numpy statement of vit_augment_u8: images [B, img, img, 3] uint8, plan [B][depth] -> the
    augmented batch (slot 0 first)."""
    images_u8 = np.asarray(images_u8)
    assert images_u8.dtype == np.uint8 and images_u8.ndim == 4 and images_u8.shape[-1] == 3
    assert len(plan) == images_u8.shape[0]
    out = np.empty_like(images_u8)
    for b, row in enumerate(plan):
        im = images_u8[b]
        for o in row:
            im = apply_op(im, o, fill)
        out[b] = im
    return out
