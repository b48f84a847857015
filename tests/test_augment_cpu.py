"""RandAugment, host side (no GPU): vit.augment.reference_apply equals Pillow byte for byte for each of
the 14 ops (include/vit_data.h); vit_randaugment_draw equals augment.reference_draw; invalid plans are
rejected before any GPU work; the new entry points are part of the bound surface."""
import ctypes
import math

import numpy as np
import pytest
from PIL import Image, ImageEnhance, ImageOps

FILLS = [(0, 0, 0), (124, 116, 104)]
FACTORS = [0.0, 0.05, 0.5, 1.0, 1.3, 1.9]


def images(img):
    """name -> [img, img, 3] uint8: uniform noise, a smooth gradient, an image with one constant
    channel (the hi <= lo and single-bin branches) and noise squeezed into [40, 125] (non-trivial
    autocontrast / equalize tables)."""
    rng = np.random.default_rng(1000 + img)
    noise = rng.integers(0, 256, (img, img, 3), dtype=np.uint8)
    y, x = np.mgrid[0:img, 0:img]
    grad = np.stack([x * 255 // (img - 1), y * 255 // (img - 1), (x + y) * 255 // (2 * img - 2)], -1).astype(np.uint8)
    const = rng.integers(0, 256, (img, img, 3), dtype=np.uint8)
    const[..., 1] = 77
    squeezed = rng.integers(40, 126, (img, img, 3), dtype=np.uint8)
    return {"noise": noise, "gradient": grad, "const_channel": const, "squeezed": squeezed}


def pil_apply(a, im, o, fill):
    kind, iarg, farg, coef = o
    p = Image.fromarray(im, "RGB")
    if kind == a.IDENTITY:
        r = p
    elif kind == a.AUTOCONTRAST:
        r = ImageOps.autocontrast(p)
    elif kind == a.EQUALIZE:
        r = ImageOps.equalize(p)
    elif kind == a.POSTERIZE:
        r = ImageOps.posterize(p, iarg)
    elif kind == a.SOLARIZE:
        r = ImageOps.solarize(p, iarg)
    elif kind == a.BRIGHTNESS:
        r = ImageEnhance.Brightness(p).enhance(farg)
    elif kind == a.CONTRAST:
        r = ImageEnhance.Contrast(p).enhance(farg)
    elif kind == a.COLOR:
        r = ImageEnhance.Color(p).enhance(farg)
    elif kind == a.SHARPNESS:
        r = ImageEnhance.Sharpness(p).enhance(farg)
    else:
        r = p.transform(p.size, Image.AFFINE, coef, Image.NEAREST, fillcolor=tuple(fill))
    return np.asarray(r)


def sweep(a, img):
    """Every (op, argument) of the issue's sweep for images of side img."""
    ops = [a.op(a.IDENTITY), a.op(a.AUTOCONTRAST), a.op(a.EQUALIZE)]
    ops += [a.op(a.POSTERIZE, iarg=b) for b in range(1, 9)]
    ops += [a.op(a.SOLARIZE, iarg=t) for t in (0, 1, 100, 255, 256)]
    ops += [a.op(k, farg=float(np.float32(f))) for k in a.ENHANCERS for f in FACTORS]
    for v in (0.09, 0.3):
        for s in (1, -1):
            ops += [a.shear_x(s * v), a.shear_y(s * v)]
    for t in (0, 3, -3, img, -img):
        ops += [a.translate_x(float(t)), a.translate_y(float(t))]
    for d in (0, 9, 30, 90):
        for s in (1, -1):
            ops.append(a.rotate(float(s * d), img))
    return ops


@pytest.mark.parametrize("img", [37, 16])
def test_reference_apply_equals_pillow(vit, img):
    a = vit.augment
    ims = images(img)
    checked = 0
    for o in sweep(a, img):
        fills = FILLS if o[0] in a.AFFINE else FILLS[:1]
        for fill in fills:
            for name, im in ims.items():
                got = a.reference_apply(im[None], [[o]], fill)[0]
                want = pil_apply(a, im, o, fill)
                assert np.array_equal(got, want), (a.OP_NAMES[o[0]], o, fill, name,
                                                   int(np.abs(got.astype(int) - want).max()))
                checked += 1
    assert checked > 300


@pytest.mark.parametrize("img", [37, 16])
def test_full_translate_is_all_fill(vit, img):
    a = vit.augment
    im = images(img)["noise"]
    for o in (a.translate_x(float(img)), a.translate_x(float(-img)), a.translate_y(float(img)),
              a.translate_y(float(-img))):
        out = a.reference_apply(im[None], [[o]], FILLS[1])[0]
        assert (out == np.asarray(FILLS[1], np.uint8)).all()


def test_tables_are_not_trivial(vit):
    """The squeezed image really exercises the autocontrast / equalize tables and the constant
    channel really is left alone (so the Pillow comparison above covers those branches)."""
    a = vit.augment
    ims = images(37)
    for kind in (a.AUTOCONTRAST, a.EQUALIZE):
        out = a.reference_apply(ims["squeezed"][None], [[a.op(kind)]])[0]
        assert (out != ims["squeezed"]).mean() > 0.5
        assert out.min() < 10 and out.max() > 245
        out = a.reference_apply(ims["const_channel"][None], [[a.op(kind)]])[0]
        assert np.array_equal(out[..., 1], ims["const_channel"][..., 1])


def c_draw(vit, seed, key, num_ops, magnitude, img):
    a = vit.augment
    out = (a.AugOp * num_ops)()
    rc = vit.lib().vit_randaugment_draw(seed, key, num_ops, magnitude, img, out)
    assert rc == 0, vit.check("draw")
    return a.plan_from_c(out, 1, num_ops)[0]


def same_op(x, y, tol=0.0):
    return x[:3] == y[:3] and all(abs(p - q) <= tol for p, q in zip(x[3], y[3]))


def test_c_draw_equals_reference_draw(vit):
    a = vit.augment
    n = 0
    for seed in (0, 1337, (1 << 64) - 3):
        for key in list(range(40)) + [10 ** 12 + 7, -5]:
            for num_ops, m, img in ((1, 0, 16), (2, 9, 224), (4, 30, 37), (3, 17, 224)):
                got = c_draw(vit, seed, key, num_ops, m, img)
                want = a.reference_draw(seed, key, num_ops, m, img)
                assert len(got) == len(want) == num_ops
                for g, w in zip(got, want):
                    # everything exact but the rotation's coefficients (libm from two languages)
                    assert same_op(g, w, 1e-12 if g[0] == a.ROTATE else 0.0), (seed, key, m, img, g, w)
                    n += 1
    assert n > 1000


def test_draw_is_keyed(vit):
    a = vit.augment
    p0 = [c_draw(vit, 7, k, 2, 9, 224) for k in range(64)]
    p1 = [c_draw(vit, 7, k, 2, 9, 224) for k in range(64)]
    assert p0 == p1
    assert len({tuple(p) for p in p0}) > 32          # different keys, different plans
    assert p0 != [c_draw(vit, 8, k, 2, 9, 224) for k in range(64)]
    # the first slots of a deeper draw are the shallower draw (slot j uses words 2j, 2j+1)
    assert c_draw(vit, 7, 5, 4, 9, 224)[:2] == p0[5]
    ra = a.RandAugment(2, 9, seed=7)
    assert ra.plan(4, 224) == [a.reference_draw(7, k, 2, 9, 224) for k in range(4)]
    assert ra.plan(4, 224) == [a.reference_draw(7, k, 2, 9, 224) for k in range(4, 8)]
    assert ra.plan(2, 224, keys=[100, 3]) == [a.reference_draw(7, 100, 2, 9, 224), a.reference_draw(7, 3, 2, 9, 224)]


def test_draw_covers_every_op_and_sign(vit):
    a = vit.augment
    seen, neg, pos = set(), set(), set()
    for key in range(4000):
        for o in c_draw(vit, 3, key, 1, 9, 224):
            seen.add(o[0])
            if o[0] in a.ENHANCERS:
                (neg if o[2] < 1 else pos).add(o[0])
            elif o[0] in a.AFFINE:
                s = sum(o[3][i] for i in (1, 2, 3, 5)) if o[0] != a.ROTATE else o[3][1]
                (neg if s < 0 else pos).add(o[0])
    signed = set(a.ENHANCERS) | set(a.AFFINE)
    assert seen == set(range(14))
    assert neg == signed and pos == signed


def test_magnitude_zero_draws_neutral_parameters(vit):
    """magnitude 0: every parameter is the neutral one (zero shear / shift / angle, factor 1, 8 bits,
    threshold 255) and reference_apply returns the input.  Two ops have no magnitude and are left out
    of the second statement: AutoContrast and Equalize; and Solarize's neutral threshold 255 still
    inverts the value 255 itself (ImageOps.solarize does too), which is asserted as such."""
    a = vit.augment
    im = images(37)["noise"]
    assert (im == 255).any()
    kinds = set()
    for key in range(300):
        for o in c_draw(vit, 11, key, 2, 0, 37):
            kinds.add(o[0])
            assert o[2] == 1.0
            assert all(abs(p - q) <= 1e-12 for p, q in zip(o[3], a.UNIT)), o
            assert o[1] == {a.POSTERIZE: 8, a.SOLARIZE: 255}.get(o[0], 0)
            out = a.reference_apply(im[None], [[o]])[0]
            if o[0] in (a.AUTOCONTRAST, a.EQUALIZE):
                continue
            if o[0] == a.SOLARIZE:
                assert np.array_equal(out, np.where(im == 255, 0, im))
            else:
                assert np.array_equal(out, im), a.OP_NAMES[o[0]]
    assert kinds == set(range(14))


def test_draw_rejects_bad_arguments(vit):
    a = vit.augment
    out = (a.AugOp * 8)()
    L = vit.lib()
    for num_ops, m, img in ((0, 9, 224), (5, 9, 224), (2, -1, 224), (2, 31, 224), (2, 9, 0)):
        assert L.vit_randaugment_draw(1, 1, num_ops, m, img, out) != 0
        with pytest.raises(vit.VitError):
            vit.check("draw")


def invalid_plans(a, img=16):
    """name -> (plan [2][depth], depth): each breaks one rule of vit_augment_u8."""
    good = a.op(a.IDENTITY)
    nan, inf = float("nan"), float("inf")
    bad = {
        "unknown op": a.op(14), "negative op": a.op(-1),
        "bits 0": a.op(a.POSTERIZE, iarg=0), "bits 9": a.op(a.POSTERIZE, iarg=9),
        "threshold -1": a.op(a.SOLARIZE, iarg=-1), "threshold 257": a.op(a.SOLARIZE, iarg=257),
        "negative factor": a.op(a.COLOR, farg=-0.1), "nan factor": a.op(a.BRIGHTNESS, farg=nan),
        "inf factor": a.op(a.SHARPNESS, farg=inf),
        "nan coefficient": a.shear_x(nan), "inf coefficient": a.translate_y(inf),
        "coefficient out of range": a.translate_x(40000.0),
    }
    out = {k: ([[good, good], [good, o]], 2) for k, o in bad.items()}
    out["depth 5"] = ([[good] * 5, [good] * 5], 5)
    return out


def test_augment_u8_rejects_invalid_plans_on_the_host(vit):
    """The plan is validated before any GPU work: with no GPU in the process, an invalid plan is
    refused with a message (a valid one would go on to the device and is not tried here)."""
    a = vit.augment
    L = vit.lib()
    fill = (ctypes.c_ubyte * 3)(0, 0, 0)
    dummy = ctypes.c_void_p(4096)  # never dereferenced: rejection comes first
    for name, (plan, depth) in invalid_plans(a).items():
        arr, batch, d = a.plan_to_c(plan)
        assert L.vit_augment_u8(dummy, batch, 16, arr, d, fill, None) != 0, name
        with pytest.raises(vit.VitError):
            vit.check(name)
    arr, batch, d = a.plan_to_c([[a.op(a.IDENTITY)]])
    for args in ((None, 1, 16, arr, 1, fill, None), (dummy, 0, 16, arr, 1, fill, None),
                 (dummy, 1, 0, arr, 1, fill, None), (dummy, 1, 16, None, 1, fill, None),
                 (dummy, 1, 16, arr, 0, fill, None), (dummy, 1, 16, arr, 1, None, None)):
        assert L.vit_augment_u8(*args) != 0
        with pytest.raises(vit.VitError):
            vit.check("arguments")


def test_public_surface(vit):
    for name in ("vit_augment_u8", "vit_randaugment_draw", "vit_trainer_set_augment_plan",
                 "vit_jpeg_loader_set_randaugment", "vit_jpeg_loader_plan"):
        assert name in vit.exported_symbols()
    assert ctypes.sizeof(vit.augment.AugOp) == 64
    assert vit.HIT_AUGMENT + 4 <= len(vit.kernel_hits())
    assert hasattr(vit, "augment_u8") and hasattr(vit.ViT, "set_augment_plan")
    assert hasattr(vit.JpegLoader, "set_randaugment") and hasattr(vit.JpegLoader, "plan")
    assert math.isclose(vit.augment.rotate(90.0, 16)[3][1], -1.0)
