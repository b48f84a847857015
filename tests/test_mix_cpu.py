"""Host side of soft-target training (vit.rs_amd/mix.py): the per-batch draw, the numpy statement
of the mix kernels and the target matrix.  No GPU."""
import math

import numpy as np


def test_mixer_same_seed_same_sequence(vit):
    a = vit.mix.Mixer(seed=7)
    b = vit.mix.Mixer(seed=7)
    sa = [a.draw(224) for _ in range(200)]
    sb = [b.draw(224) for _ in range(200)]
    assert sa == sb
    c = vit.mix.Mixer(seed=8)
    assert [c.draw(224) for _ in range(200)] != sa


def test_mixer_default_draws_are_valid(vit):
    img, n = 224, 2000
    m = vit.mix.Mixer()
    modes = []
    for _ in range(n):
        mode, lam, box = m.draw(img)
        assert mode in (vit.mix.MIX_MIXUP, vit.mix.MIX_CUTMIX)  # prob = 1
        assert 0.0 <= lam <= 1.0
        if mode == vit.mix.MIX_CUTMIX:
            x0, y0, x1, y1 = box
            assert 0 <= x0 <= x1 <= img and 0 <= y0 <= y1 <= img
            assert lam == vit.mix.cutmix_lam(box, img)
        else:
            assert box is None
        modes.append(mode)
    share = np.mean(np.array(modes) == vit.mix.MIX_CUTMIX)
    sd = math.sqrt(m.switch_prob * (1 - m.switch_prob) / n)
    assert abs(share - m.switch_prob) <= 5 * sd, share


def test_mixer_prob_zero_and_no_cutmix(vit):
    m = vit.mix.Mixer(prob=0.0, seed=1)
    assert all(m.draw(32) == (vit.mix.MIX_NONE, 1.0, None) for _ in range(200))
    m = vit.mix.Mixer(cutmix_alpha=0.0, seed=2)
    assert all(m.draw(32)[0] == vit.mix.MIX_MIXUP for _ in range(500))
    m = vit.mix.Mixer(mixup_alpha=0.0, seed=3)
    assert all(m.draw(32)[0] == vit.mix.MIX_CUTMIX for _ in range(500))
    m = vit.mix.Mixer(mixup_alpha=0.0, cutmix_alpha=0.0, seed=4)
    assert all(m.draw(32)[0] == vit.mix.MIX_NONE for _ in range(50))


def _batch(B, img=8, seed=0):
    rng = np.random.RandomState(seed)
    return rng.randn(B, 3, img, img).astype(np.float32), rng.randint(0, 10, B).astype(np.int32)


def test_reference_mix_odd_batch_keeps_middle_image(vit):
    px, lab = _batch(5)
    for mode, lam, box in ((vit.mix.MIX_MIXUP, 0.3, None), (vit.mix.MIX_CUTMIX, 1.0, (1, 2, 6, 7))):
        out, ta, tb, _ = vit.mix.reference_mix(px, lab, mode, lam, box)
        assert out.dtype == np.float32
        assert np.array_equal(out[2].view(np.uint32), px[2].view(np.uint32))
        assert not np.array_equal(out[0], px[0])
        assert np.array_equal(ta, lab) and np.array_equal(tb, lab[::-1])
    # the mixup arithmetic, element by element, each operation rounded to fp32
    out, _, _, lam_used = vit.mix.reference_mix(px, lab, vit.mix.MIX_MIXUP, 0.3)
    lam = np.float32(0.3)
    oml = np.float32(1.0) - lam
    assert lam_used == float(lam)
    want = np.float32(lam * px[0, 1, 2, 3]) + np.float32(oml * px[4, 1, 2, 3])
    assert out[0, 1, 2, 3] == np.float32(want)
    want = np.float32(lam * px[4, 1, 2, 3]) + np.float32(oml * px[0, 1, 2, 3])
    assert out[4, 1, 2, 3] == np.float32(want)


def test_reference_mix_empty_and_full_box(vit):
    px, lab = _batch(4)
    out, ta, tb, lam = vit.mix.reference_mix(px, lab, vit.mix.MIX_CUTMIX, 0.5, (3, 3, 3, 7))
    assert np.array_equal(out, px) and lam == 1.0
    out, ta, tb, lam = vit.mix.reference_mix(px, lab, vit.mix.MIX_CUTMIX, 0.5, (0, 0, 8, 8))
    assert np.array_equal(out, px[::-1]) and lam == 0.0
    assert np.array_equal(ta, lab) and np.array_equal(tb, lab[::-1])
    out, ta, tb, lam = vit.mix.reference_mix(px, lab, vit.mix.MIX_NONE)
    assert np.array_equal(out, px) and lam == 1.0 and np.array_equal(ta, tb)


def test_soft_targets(vit):
    ta = np.array([0, 3, 3, 9])
    tb = ta[::-1]
    for lam in (1.0, 0.3, 0.0):
        for eps in (0.0, 0.1):
            t = vit.mix.soft_targets(ta, tb, lam, eps, 10)
            assert t.dtype == np.float64 and t.shape == (4, 10)
            # lam + (1 - lam in fp32) is 1 to within one fp32 rounding
            assert np.abs(t.sum(axis=1) - 1.0).max() <= 2.0 ** -24
            assert t.min() >= 0
    t = vit.mix.soft_targets(ta, tb, 1.0, 0.0, 10)
    assert np.array_equal(t, np.eye(10)[ta])
    assert np.array_equal(vit.mix.soft_targets(ta, None, 0.3, 0.0, 10), np.eye(10)[ta])
    t = vit.mix.soft_targets(ta, tb, 0.25, 0.5, 10)
    assert abs(t[0, 0] - (0.5 * 0.25 + 0.05)) < 1e-12 and abs(t[0, 9] - (0.5 * 0.75 + 0.05)) < 1e-12
    assert abs(t[1, 3] - (0.5 + 0.05)) < 1e-12  # rows 1 and 2 are partners with the same label
