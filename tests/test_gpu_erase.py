"""Random erasing on the device fp32 batch (erase.hip) against vit.erase.reference_apply (numpy float64): the op
on hand-made boxes in all three modes, position independence (device against device), the trainer call with
its ordering and states, the launch counters of the unused feature and the op's rejections."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODES = (0, 1, 2)  # CONST, RAND, PIXEL
SEED = 2 ** 63 + 12345


def hand_boxes(img, B):
    """[B, 2, 4], B >= 3: image 0 a full-height one-column box and, overlapping it, a box that touches the
    right and bottom edges (x1 = y1 = img); image 1 no box; image 2 a 1 x 1 box and an empty box (zero width);
    3 (if any) two overlapping boxes inside the image; 4 (if any) the whole image but one row, beside an empty
    box of zero height."""
    b = np.zeros((B, 2, 4), np.int32)
    b[0] = [[img - 1, 0, img, img], [img - 5, img - 3, img, img]]
    b[2] = [[5, 6, 6, 7], [4, 2, 4, 9]]
    if B > 3:
        b[3] = [[2, 3, 11, 9], [7, 5, 14, 13]]
    if B > 4:
        b[4] = [[0, 1, img, img], [3, 8, 9, 8]]
    return b


def case(img, B, seed=0):
    rng = np.random.default_rng(seed)
    px = rng.standard_normal((B, 3, img, img)).astype(np.float32)
    keys = (np.arange(B, dtype=np.int64) + 1) * 1000003 - 17
    return px, hand_boxes(img, B), keys


def run(v, px, boxes, mode, seed=SEED, keys=None):
    d = v.DeviceArray.from_numpy(px)
    try:
        v.random_erase(d, boxes, mode, seed, keys)
        return d.numpy()
    finally:
        d.free()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_against_reference(v, got, px, boxes, mode, seed, keys, what):
    """Criterion 1: outside the boxes the input's bits; CONST the reference's bits; RAND and PIXEL within one
    fp32 ulp of the float64 reference rounded to fp32, or 1e-15 absolute, whichever is larger.  Returns the
    number of elements that are not bit-equal to the rounded reference."""
    er = v.erase
    B, img = px.shape[0], px.shape[-1]
    ref64 = er.reference_apply(px, boxes, mode, seed, keys)
    ref = ref64.astype(np.float32)
    inside = np.broadcast_to(er.inside_mask(boxes, B, img), px.shape)
    assert np.array_equal(bits(got)[~inside], bits(px)[~inside]), f"{what}: a pixel outside the boxes changed"
    if mode == er.ERASE_CONST:
        assert np.array_equal(bits(got), bits(ref)), what
        return 0
    diff = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    tol = np.maximum(np.spacing(np.abs(ref)).astype(np.float64), 1e-15)
    unequal = int((bits(got) != bits(ref)).sum())
    print(f"{what}: {int(inside.sum())} erased elements, {unequal} not bit-equal to the rounded float64 reference, "
          f"max |diff| / tol {float((diff / tol).max()):.3f}")
    assert np.all(diff <= tol), (what, float((diff / tol).max()))
    return unequal


# ------------------------------------------------------------------ 1. the op against the reference
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("img,B", [(37, 5), (16, 3)])
def test_op_equals_reference(gpu, img, B, mode):
    v = gpu
    px, boxes, keys = case(img, B)
    got = run(v, px, boxes, mode, SEED, keys)
    check_against_reference(v, got, px, boxes, mode, SEED, keys, f"img {img} B {B} mode {mode}")
    if mode != v.ERASE_CONST:
        inside = np.broadcast_to(v.erase.inside_mask(boxes, B, img), px.shape)
        assert np.all(got[inside] != px[inside])  # every covered pixel was written
    if mode == v.ERASE_CONST:  # CONST needs no keys
        assert np.array_equal(bits(run(v, px, boxes, mode, 0, None)), bits(got))


# ------------------------------------------------------------------ 2. position independence, exact
@pytest.mark.parametrize("mode", [1, 2])
def test_key_gives_the_same_image_in_any_slot(gpu, mode):
    v = gpu
    img = 37
    px, boxes, keys = case(img, 5, seed=4)
    one_px = px[3:4].copy()
    one_boxes = np.array([[[3, 1, 20, 30], [10, 12, 37, 29]]], np.int32)
    key = np.array([424242], np.int64)
    alone = run(v, one_px, one_boxes, mode, SEED, key)
    px[3], boxes[3], keys[3] = one_px[0], one_boxes[0], key[0]
    big = run(v, px, boxes, mode, SEED, keys)
    assert np.array_equal(bits(big[3]), bits(alone[0]))
    assert not np.array_equal(bits(big[3]), bits(px[3]))


def test_pixel_values_in_an_overlap_equal_either_box_alone(gpu):
    v = gpu
    img = 37
    px, boxes, keys = case(img, 5, seed=5)
    both = run(v, px, boxes, v.ERASE_PIXEL, SEED, keys)
    for k in range(2):
        one = boxes.copy()
        one[0, 1 - k] = 0
        alone = run(v, px, one, v.ERASE_PIXEL, SEED, keys)
        x0, y0, x1, y1 = boxes[0, k]
        assert np.array_equal(bits(both[0, :, y0:y1, x0:x1]), bits(alone[0, :, y0:y1, x0:x1]))
        assert np.array_equal(bits(both[1:]), bits(alone[1:]))


# ------------------------------------------------------------------ 3. the trainer
def trainer_cfg(v, prec):
    """img 32, patch 8 in both: `test` (head size 16) for fp32 mode; the bf16 path needs a head size of 32 or
    more, so bf16 mode runs `test_h64`, the same geometry with 128 channels."""
    return v.data.CONFIGS["test" if prec == v.VIT_FP32 else "test_h64"]


def trainer_case(v, prec, B=4, seed=7):
    cfg = trainer_cfg(v, prec)
    px, lab = v.data.synthetic_batch(cfg, B, seed=seed)
    boxes = np.zeros((B, 2, 4), np.int32)
    boxes[0] = [[2, 3, 11, 9], [7, 5, 14, 13]]
    boxes[1, 1] = [cfg.img - 5, cfg.img - 3, cfg.img, cfg.img]
    boxes[3] = [[0, 0, 1, 1], [31, 0, 32, 32]]
    keys = np.arange(B, dtype=np.int64) * 31 + 5
    return cfg, px, lab, boxes, keys


@pytest.fixture(scope="module")
def models(gpu):
    v = gpu
    ms = {}
    for p in (v.VIT_FP32, v.VIT_BF16):
        cfg = trainer_cfg(v, p)
        ms[p] = v.ViT.build(cfg, 4, p, params=v.data.init_params(cfg, "parity", seed=3))
    yield ms
    for m in ms.values():
        m.close()


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("mode", MODES)
def test_trainer_erase_then_mix_then_forward(gpu, models, prec, mode):
    v = gpu
    m = models[prec]
    cfg, px, lab, boxes, keys = trainer_case(v, prec)
    m.set_batch(px, lab)
    m.erase_batch(boxes, mode, SEED, keys)
    erased = m.pixels()
    check_against_reference(v, erased, px, boxes, mode, SEED, keys, f"trainer prec {prec} mode {mode}")
    # forward of the erased batch == forward of a fresh upload of the pixels read back
    loss = m.forward()
    logits = m.logits()
    loss2 = m.forward(erased, lab)
    assert np.float32(loss).view(np.uint32) == np.float32(loss2).view(np.uint32)
    assert np.array_equal(bits(logits), bits(m.logits()))
    # erase first, then mix: the mix of the erased pixels, bit for bit
    for mix_mode, lam, box in ((v.MIX_MIXUP, 0.3, None), (v.MIX_CUTMIX, 1.0, (4, 6, 20, 30))):
        m.set_batch(px, lab)
        m.erase_batch(boxes, mode, SEED, keys)
        m.mix_batch(mix_mode, lam, box)
        want, _, _, _ = v.mix.reference_mix(erased, lab, mix_mode, lam, box)
        assert np.array_equal(bits(m.pixels()), bits(want)), (mode, mix_mode)


@pytest.mark.parametrize("prec", [0, 1])
def test_trainer_erase_is_ordered_behind_the_u8_normalise(gpu, models, prec):
    v = gpu
    m = models[prec]
    cfg, _, lab, boxes, keys = trainer_case(v, prec)
    images = np.random.default_rng(1).integers(0, 256, (4, cfg.img, cfg.img, 3), dtype=np.uint8)
    m.set_batch_u8(images, lab)
    normalised = m.pixels()
    for mode in (v.ERASE_CONST, v.ERASE_PIXEL):
        m.set_batch_u8(images, lab)
        m.erase_batch(boxes, mode, SEED, keys)
        got = m.pixels()
        check_against_reference(v, got, normalised, boxes, mode, SEED, keys, f"u8 path prec {prec} mode {mode}")
        inside = np.broadcast_to(v.erase.inside_mask(boxes, 4, cfg.img), got.shape)
        assert not np.array_equal(bits(got)[inside], bits(normalised)[inside])


@pytest.mark.parametrize("prec", [0, 1])
def test_trainer_states_and_errors(gpu, models, prec):
    v = gpu
    m = models[prec]
    cfg, px, lab, boxes, keys = trainer_case(v, prec)

    def refused(text, *args):
        before = m.pixels()
        with pytest.raises(v.VitError, match=text):
            m.erase_batch(*args)
        assert np.array_equal(bits(m.pixels()), bits(before))

    # erase after mix
    m.set_batch(px, lab)
    m.mix_batch(v.MIX_MIXUP, 0.4)
    refused("already mixed", boxes, v.ERASE_PIXEL, SEED, keys)
    # a second erase (also after an erase whose boxes were all empty)
    m.set_batch(px, lab)
    m.erase_batch(boxes, v.ERASE_PIXEL, SEED, keys)
    refused("already erased", boxes, v.ERASE_CONST, SEED, keys)
    m.set_batch(px, lab)
    m.erase_batch(np.zeros_like(boxes), v.ERASE_PIXEL, SEED, keys)
    refused("already erased", boxes, v.ERASE_PIXEL, SEED, keys)
    # a bad box leaves the batch and the states as they were: the next erase is the first
    m.set_batch(px, lab)
    bad = boxes.copy()
    bad[2, 1] = [3, 3, cfg.img + 1, 5]
    refused("outside", bad, v.ERASE_PIXEL, SEED, keys)
    refused("host_keys", boxes, v.ERASE_PIXEL, SEED, None)
    assert np.array_equal(bits(m.pixels()), bits(px))
    m.erase_batch(boxes, v.ERASE_PIXEL, SEED, keys)
    first = m.pixels()
    # set_batch clears both states
    m.mix_batch(v.MIX_MIXUP, 0.4)
    m.set_batch(px, lab)
    m.erase_batch(boxes, v.ERASE_PIXEL, SEED, keys)
    assert np.array_equal(bits(m.pixels()), bits(first))
    # a batch without labels can be erased
    m.set_batch(px, None)
    m.erase_batch(boxes, v.ERASE_RAND, SEED, keys)
    check_against_reference(v, m.pixels(), px, boxes, v.ERASE_RAND, SEED, keys, "no labels")
    assert m.forward() == -1.0


# ------------------------------------------------------------------ 4. the unused feature
def test_unused_feature_launches_nothing(gpu):
    v = gpu
    cfg = v.data.CONFIGS["test_h64"]
    B = 4
    params = v.data.init_params(cfg, "parity", seed=4)
    px, lab = v.data.synthetic_batch(cfg, B, seed=5)
    keys = np.arange(B, dtype=np.int64)
    boxes = np.zeros((B, 1, 4), np.int32)

    def step(erase):
        m = v.ViT.build(cfg, B, v.VIT_BF16, params=params)
        bytes0 = m.device_bytes()
        v.kernel_hits_reset()
        m.set_batch(px, lab)
        if erase is not None:
            m.erase_batch(erase, v.ERASE_PIXEL, SEED, keys)
        m.train_step(1e-3)
        m.sync()
        hits, grew, p = v.kernel_hits(), m.device_bytes() - bytes0, m.params()
        m.close()
        return hits, grew, p

    plain, grew0, p0 = step(None)
    assert plain[v.HIT_ERASE] == 0 and plain.sum() > 0
    # boxes that are all empty: returns 0, launches nothing, allocates nothing, the same step
    empty, grew1, p1 = step(boxes)
    assert np.array_equal(empty, plain) and grew1 == grew0
    assert np.array_equal(bits(p1), bits(p0))
    # one box: one launch in the erase family and no other counter moves
    boxes[2, 0] = [3, 4, 9, 11]
    used, grew2, p2 = step(boxes)
    want = plain.copy()
    want[v.HIT_ERASE] = 1
    assert np.array_equal(used, want), np.nonzero(used != want)
    assert grew2 > grew0 and not np.array_equal(bits(p2), bits(p0))
    # the op itself: a call whose boxes are all empty returns 0 and launches nothing
    v.kernel_hits_reset()
    got = run(v, px, np.zeros((B, 3, 4), np.int32), v.ERASE_PIXEL, SEED, keys)
    assert v.kernel_hits().sum() == 0 and np.array_equal(bits(got), bits(px))
    run(v, px, boxes, v.ERASE_CONST)
    assert v.kernel_hits()[v.HIT_ERASE] == 1 and v.kernel_hits().sum() == 1


# ------------------------------------------------------------------ 5. rejections of the op
def test_op_rejections_leave_the_batch_unchanged(gpu):
    v = gpu
    img, B = 16, 3
    px, boxes, keys = case(img, B)
    d = v.DeviceArray.from_numpy(px)

    def refused(text, bx, mode, ks):
        v.kernel_hits_reset()
        with pytest.raises(v.VitError, match=text):
            v.random_erase(d, bx, mode, SEED, ks)
        assert v.kernel_hits().sum() == 0
        assert np.array_equal(bits(d.numpy()), bits(px))

    for bad in ([0, 0, img + 1, 4], [0, 0, 4, img + 1], [-1, 0, 4, 4], [0, -2, 4, 4]):  # out of range
        b = boxes.copy()
        b[2, 1] = bad
        refused("outside", b, v.ERASE_PIXEL, keys)
    for bad in ([5, 0, 4, 4], [0, 9, 4, 8]):  # x0 > x1, y0 > y1
        b = boxes.copy()
        b[0, 0] = bad
        refused("outside", b, v.ERASE_CONST, None)
    refused("unknown mode", boxes, 3, keys)
    refused("unknown mode", boxes, -1, keys)
    refused("max_count", np.zeros((B, 0, 4), np.int32), v.ERASE_CONST, None)
    refused("max_count", np.zeros((B, 5, 4), np.int32), v.ERASE_CONST, None)
    refused("host_keys", boxes, v.ERASE_PIXEL, None)
    refused("host_keys", boxes, v.ERASE_RAND, None)
    # and the same call with good arguments then works
    v.random_erase(d, boxes, v.ERASE_PIXEL, SEED, keys)
    check_against_reference(v, d.numpy(), px, boxes, v.ERASE_PIXEL, SEED, keys, "after the rejections")
    d.free()
