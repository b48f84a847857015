"""RandAugment on the device uint8 batch (augment.hip) against vit.augment.reference_apply, which
tests/test_augment_cpu.py pins to Pillow: every op alone (a different op or argument per image in
one launch, odd and even image sizes), chains of 3 and 4 ops, rejection, the trainer's one-shot
plan, the JPEG loader's per-record draw, and the launch counters of the unused feature."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "oracle"))
import jpeg_fixtures as jf  # noqa: E402
import jpeg_ref  # noqa: E402
import test_augment_cpu as tc  # noqa: E402  (the shared images, sweep and invalid plans)

pytestmark = pytest.mark.gpu

KINDS = ("noise", "gradient", "const_channel", "squeezed")


def batch_of(img, B, shift=0):
    ims = tc.images(img)
    return np.stack([ims[KINDS[(i + shift) % 4]] for i in range(B)])


def run(v, images, plan, fill=(0, 0, 0)):
    d = v.DeviceArray.from_numpy(images)
    v.augment_u8(d, plan, fill)
    out = d.numpy()
    d.free()
    return out


def aug_hits(v):
    return v.kernel_hits()[v.HIT_AUGMENT:v.HIT_AUGMENT + 4]


@pytest.mark.parametrize("img,B", [(37, 5), (16, 3)])
def test_single_ops_equal_reference(gpu, img, B):
    """depth 1, a different op or argument per image in one launch, over the whole sweep of the CPU
    test (all 14 ops), both fill colours, each op on several of the four image kinds."""
    v, a = gpu, gpu.augment
    ops = tc.sweep(a, img)
    seen = set()
    for fill in tc.FILLS:
        for g in range(0, len(ops), B):
            group = [ops[(g + i) % len(ops)] for i in range(B)]
            images = batch_of(img, B, shift=g // B)
            plan = [[o] for o in group]
            got = run(v, images, plan, fill)
            want = a.reference_apply(images, plan, fill)
            for i in range(B):
                assert np.array_equal(got[i], want[i]), (a.OP_NAMES[group[i][0]], group[i], fill, i)
                seen.add(group[i][0])
    assert seen == set(range(14))


@pytest.mark.parametrize("img", [37, 16])
def test_table_ops_on_every_image_kind(gpu, img):
    """autocontrast, equalize and contrast (the ops with image statistics) on each image kind: the
    squeezed image (non-trivial tables) and the constant channel (hi <= lo, single bin) included."""
    v, a = gpu, gpu.augment
    images = batch_of(img, 4)
    for o in (a.op(a.AUTOCONTRAST), a.op(a.EQUALIZE), a.op(a.CONTRAST, farg=0.5), a.op(a.CONTRAST, farg=1.9)):
        plan = [[o]] * 4
        got = run(v, images, plan)
        want = a.reference_apply(images, plan)
        for i in range(4):
            assert np.array_equal(got[i], want[i]), (a.OP_NAMES[o[0]], KINDS[i])
    # (at img = 16 equalize takes its step == 0 branch: 256 pixels leave step = 0)
    changed = not np.array_equal(a.reference_apply(images, [[a.op(a.EQUALIZE)]] * 4)[3], images[3])
    assert changed == (img == 37)


def chain_plans(a, img):
    I = a.op(a.IDENTITY)
    f = lambda k, x: a.op(k, farg=float(np.float32(x)))  # noqa: E731
    d3 = [[a.rotate(30.0, img), I, f(a.SHARPNESS, 1.9)],                  # identity in the middle, sharpness after affine
          [a.shear_x(0.3), a.translate_y(3.0), f(a.COLOR, 0.5)],          # two geometric ops in a row
          [a.op(a.EQUALIZE), I, a.rotate(-9.0, img)],                     # ends in the scratch buffer
          [f(a.SHARPNESS, 0.05), a.shear_y(-0.09), a.op(a.AUTOCONTRAST)],  # statistics read from the right buffer
          [a.op(a.SOLARIZE, iarg=100), f(a.CONTRAST, 1.3), a.op(a.POSTERIZE, iarg=3)]]
    d4 = [[a.translate_x(3.0), a.rotate(9.0, img), f(a.SHARPNESS, 1.3), f(a.BRIGHTNESS, 0.5)],
          [I, I, I, I],
          [f(a.CONTRAST, 0.5), a.shear_x(-0.3), a.shear_y(0.3), a.op(a.EQUALIZE)],
          [f(a.COLOR, 1.9), I, f(a.SHARPNESS, 0.0), a.rotate(90.0, img)],
          [a.op(a.AUTOCONTRAST), a.op(a.EQUALIZE), a.op(a.POSTERIZE, iarg=2), a.op(a.SOLARIZE, iarg=1)]]
    return {3: d3, 4: d4}


@pytest.mark.parametrize("depth", [3, 4])
@pytest.mark.parametrize("img", [37, 16])
def test_chains_equal_reference_and_repeat(gpu, img, depth):
    v, a = gpu, gpu.augment
    plan = chain_plans(a, img)[depth]
    images = batch_of(img, 5, shift=1)
    fill = tc.FILLS[1]
    got = run(v, images, plan, fill)
    want = a.reference_apply(images, plan, fill)
    for i in range(5):
        assert np.array_equal(got[i], want[i]), (depth, i)
    assert np.array_equal(run(v, images, plan, fill), got)


def test_rejection_leaves_images_intact(gpu):
    v, a = gpu, gpu.augment
    images = batch_of(16, 2)
    d = v.DeviceArray.from_numpy(images)
    for name, (plan, depth) in tc.invalid_plans(a).items():
        with pytest.raises(v.VitError):
            v.augment_u8(d, plan)
        assert np.array_equal(d.numpy(), images), name
    # a plan whose last image is the bad one: nothing of the good images' ops has run either
    plan = [[a.op(a.SOLARIZE, iarg=0)], [a.op(a.POSTERIZE, iarg=0)]]
    with pytest.raises(v.VitError, match="posterize bits 0"):
        v.augment_u8(d, plan)
    assert np.array_equal(d.numpy(), images)
    v.augment_u8(d, [[a.op(a.SOLARIZE, iarg=0)]] * 2)
    assert np.array_equal(d.numpy(), 255 - images)
    d.free()


def test_trainer_one_shot_plan(gpu):
    """set_augment_plan + set_batch_u8 -> pixels() = normalise(reference_apply(images)); the next
    set_batch_u8 is unaugmented; three rounds, so both staging slots carry both kinds of batch.
    Invalid plans are rejected by set_augment_plan itself and leave nothing pending."""
    v, a = gpu, gpu.augment
    cfg = v.data.CONFIGS["test"]
    B, img = 5, cfg.img
    m = v.ViT.build(cfg, B, v.VIT_FP32, params=v.data.init_params(cfg, "parity", seed=2))
    bytes_before = m.device_bytes()
    rng = np.random.default_rng(5)
    plans = [chain_plans(a, img)[3], chain_plans(a, img)[4], [[o] for o in tc.sweep(a, img)[20:25]]]
    for r, plan in enumerate(plans):
        fill = tc.FILLS[r % 2]
        images = rng.integers(0, 256, (B, img, img, 3), dtype=np.uint8)
        labels = rng.integers(0, cfg.num_classes, B).astype(np.int32)
        m.set_augment_plan(plan, fill)
        m.set_batch_u8(images, labels)
        want = jpeg_ref.normalise(a.reference_apply(images, plan, fill), v.IMAGENET_MEAN, v.IMAGENET_STD)
        assert np.array_equal(m.pixels(), want), r
        images2 = rng.integers(0, 256, (B, img, img, 3), dtype=np.uint8)
        m.set_batch_u8(images2, labels)
        assert np.array_equal(m.pixels(), jpeg_ref.normalise(images2, v.IMAGENET_MEAN, v.IMAGENET_STD)), r
    assert m.device_bytes() > bytes_before  # the scratch is the trainer's own allocation
    images = rng.integers(0, 256, (B, img, img, 3), dtype=np.uint8)
    for name, (plan, depth) in tc.invalid_plans(a).items():
        bad = [plan[1]] * B
        with pytest.raises(v.VitError):
            m.set_augment_plan(bad)
    m.set_batch_u8(images)
    assert np.array_equal(m.pixels(), jpeg_ref.normalise(images, v.IMAGENET_MEAN, v.IMAGENET_STD))
    # None clears a pending plan
    m.set_augment_plan([[a.op(a.SOLARIZE, iarg=0)]] * B)
    m.set_augment_plan(None)
    m.set_batch_u8(images)
    assert np.array_equal(m.pixels(), jpeg_ref.normalise(images, v.IMAGENET_MEAN, v.IMAGENET_STD))
    assert np.isfinite(m.forward())
    m.close()


@pytest.fixture(scope="module")
def records(gpu, tmp_path_factory):
    jpegs, _ = jf.dataset(8, seed=21, sizes=((40, 56), (75, 50), (64, 64)))
    labels = np.arange(8, dtype=np.int32)  # the label names the record
    return gpu.write_jpeg_records(str(tmp_path_factory.mktemp("aug") / "ra"), jpegs, labels)


def test_jpeg_loader_randaugment(gpu, records):
    v, a = gpu, gpu.augment
    seed, N, B, img = 9, 8, 4, 37
    plain = v.JpegLoader(*records, batch=B, seed=seed, shuffle=True, augment=True, threads=2)
    ra = v.JpegLoader(*records, batch=B, seed=seed, shuffle=True, augment=True, threads=2)
    fill = tc.FILLS[1]
    ra.set_randaugment(2, 9, fill)
    by_record = {}
    changed = 0
    for step in range(4):  # two epochs
        lab0, ep0, _ = plain.next()
        lab1, ep1, _ = ra.next()
        assert np.array_equal(lab0, lab1) and ep0 == ep1
        assert np.array_equal(plain.boxes(), ra.boxes())  # the crop draw does not move
        assert plain.plan(img) == []
        plan = ra.plan(img)
        for i, rec in enumerate(lab1):
            want = a.reference_draw(seed, ep1 * N + int(rec), 2, 9, img)
            assert all(tc.same_op(g, w, 1e-12 if g[0] == a.ROTATE else 0.0) for g, w in zip(plan[i], want))
            by_record[(ep1, int(rec))] = plan[i]
        base = plain.decode_u8(img).numpy()
        got = ra.decode_u8(img).numpy()
        assert np.array_equal(got, a.reference_apply(base, plan, fill)), step
        changed += int((got != base).any())
    assert changed > 0
    # off again: the plain decode
    ra.set_randaugment(0, 0, fill)
    lab0, _, _ = plain.next()
    ra.next()
    assert np.array_equal(ra.decode_u8(img).numpy(), plain.decode_u8(img).numpy())
    plain.close(); ra.close()
    # the plan follows (seed, epoch, record), not rank, world size or batch position
    for rank in (0, 1):
        L = v.JpegLoader(*records, batch=2, seed=seed, rank=rank, world=2, shuffle=True, augment=True, threads=1)
        L.set_randaugment(2, 9, fill)
        for step in range(4):
            lab, ep, _ = L.next()
            for i, rec in enumerate(lab):
                assert L.plan(img)[i] == by_record[(ep, int(rec))]
        L.close()


def test_unused_feature_launches_nothing(gpu, records):
    v, a = gpu, gpu.augment
    cfg = v.data.CONFIGS["test_h64"]
    B = 4
    m = v.ViT.build(cfg, B, v.VIT_BF16, params=v.data.init_params(cfg, "parity", seed=4))
    L = v.JpegLoader(*records, batch=B, seed=1, shuffle=True, augment=True, threads=2)
    images = np.random.default_rng(0).integers(0, 256, (B, cfg.img, cfg.img, 3), dtype=np.uint8)
    v.kernel_hits_reset()
    m.set_batch_u8(images)
    L.next()
    m.set_batch_jpeg(L)
    m.sync()
    assert aug_hits(v).sum() == 0
    m.set_augment_plan([[a.op(a.IDENTITY)]] * B)  # identities launch nothing either
    m.set_batch_u8(images)
    assert aug_hits(v).sum() == 0
    m.set_augment_plan([[a.op(a.EQUALIZE), a.rotate(9.0, cfg.img)]] * B)
    m.set_batch_u8(images)
    m.sync()
    assert list(aug_hits(v)) == [1, 1, 1, 1]  # table, lookup, rotate, copy back
    # the whole recipe on the device: JPEG coefficients -> RandAugment -> mix -> train step
    L.set_randaugment(2, 9)
    v.kernel_hits_reset()
    for step in range(3):
        L.next()
        m.set_batch_jpeg(L)
        m.mix_batch(v.MIX_MIXUP, 0.3)
        m.train_step(1e-3)
    m.sync()
    assert np.isfinite(float(v.lib().vit_trainer_mean_loss(m.h)))
    assert aug_hits(v).sum() > 0
    L.close(); m.close()
