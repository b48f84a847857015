"""Soft-target training on the GPU: the soft-target loss ops, the in-place mixup / cutmix kernels
and the trainer paths that use them (include/vit_ops.h, include/vit_trainer.h).

References: numpy float64 for the ops, vit.mix.reference_mix (numpy fp32, bit for bit) for the mix
kernels, and the CPU oracle for the trainer: the loss is linear in the target and lam is one number
per batch, so with px' the mixed pixels the soft-target loss / gradient is
    (1-eps) (lam X_a + oml X_b) + (eps/V) sum_k X_k
of the oracle's hard-label passes on px' (a: the labels, b: the reversed labels, k: label k on
every row), 2 + V passes.  Gates are the project's own (tests/parity.py)."""
import functools

import numpy as np
import pytest

import parity

pytestmark = pytest.mark.gpu


def D(v, a, dt=np.float32):
    return v.DeviceArray.from_numpy(np.asarray(a), dt)


def Z(v, n, dt=np.float32):
    return v.DeviceArray.zeros(n, dt)


def lse64(z):
    m = z.max(axis=1, keepdims=True)
    return (m + np.log(np.exp(z - m).sum(axis=1, keepdims=True)))[:, 0]


def op_case(rows, V, given_tb):
    rng = np.random.default_rng(1000 * rows + V)
    z = (rng.normal(size=(rows, V)) * 3).astype(np.float32)
    ta = rng.integers(0, V, size=rows).astype(np.int32)
    tb = rng.integers(0, V, size=rows).astype(np.int32) if given_tb else None
    return z, ta, tb


SHAPES = [(5, 10), (3, 7), (4, 257), (2, 1000)]


# ------------------------------------------------------------------ ops
@pytest.mark.parametrize("given_tb", [False, True])
@pytest.mark.parametrize("lam", [1.0, 0.3])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("rows,V", SHAPES)
def test_soft_forward_op(gpu, vit, rows, V, eps, lam, given_tb):
    v = gpu
    z, ta, tb = op_case(rows, V, given_tb)
    t = vit.mix.soft_targets(ta, tb, lam, eps, V)
    z64 = z.astype(np.float64)
    ref = lse64(z64) - (t * z64).sum(axis=1)
    gz, gta = D(v, z), D(v, ta, np.int32)
    gtb = D(v, tb, np.int32) if given_tb else None
    probs, losses = Z(v, rows * V), Z(v, rows)
    v.call("softmax_crossentropy_soft_forward", probs, losses, gz, gta, gtb, lam, eps, rows, 1, V)
    got = losses.numpy().astype(np.float64)
    err = np.abs(got - ref) / np.abs(ref)
    print(f"\nsoft fwd rows {rows} V {V} eps {eps} lam {lam} tb {given_tb}: max rel {err.max():.2e} "
          f"(min |ref| {np.abs(ref).min():.3e})")
    assert np.all(err <= parity.FP32["loss"]), (err, ref)
    plain = Z(v, rows * V)
    v.call("softmax_forward", plain, gz, rows, 1, V)
    assert np.array_equal(probs.numpy().view(np.uint32), plain.numpy().view(np.uint32))
    # losses NULL: a plain softmax
    p2 = Z(v, rows * V)
    v.call("softmax_crossentropy_soft_forward", p2, None, gz, gta, gtb, lam, eps, rows, 1, V)
    assert np.array_equal(p2.numpy().view(np.uint32), plain.numpy().view(np.uint32))
    if eps == 0.0 and lam == 1.0:
        hard = Z(v, rows)
        v.call("crossentropy_forward", hard, plain, gta, rows, 1, V)
        h = hard.numpy().astype(np.float64)
        e2 = np.abs(got - h) / np.abs(h)
        print(f"   vs crossentropy_forward: max rel {e2.max():.2e}")
        assert np.all(e2 <= parity.FP32["loss"]), e2


def test_soft_forward_underflowing_probability_is_finite(gpu, vit):
    """A class 200 below the maximum has probability 0 in fp32; with smoothing it has weight, and
    the loss (from the logits) stays finite and right."""
    v = gpu
    z = np.zeros((2, 10), np.float32)
    z[0, 3], z[1, 7] = 200.0, -200.0
    ta = np.array([3, 7], np.int32)
    t = vit.mix.soft_targets(ta, None, 1.0, 0.1, 10)
    ref = lse64(z.astype(np.float64)) - (t * z).sum(axis=1)
    probs, losses = Z(v, 20), Z(v, 2)
    v.call("softmax_crossentropy_soft_forward", probs, losses, D(v, z), D(v, ta, np.int32), None, 1.0, 0.1,
           2, 1, 10)
    got = losses.numpy()
    assert probs.numpy().min() == 0.0
    assert np.all(np.isfinite(got))
    assert np.all(np.abs(got - ref) <= parity.FP32["loss"] * np.abs(ref)), (got, ref)


@pytest.mark.parametrize("which", ["ta", "tb"])
@pytest.mark.parametrize("bad", [-1, 10, 1 << 30])
def test_soft_forward_out_of_range_label_is_nan_in_its_row(gpu, which, bad):
    v = gpu
    rows, V = 5, 10
    z, ta, tb = op_case(rows, V, True)
    (ta if which == "ta" else tb)[2] = bad
    probs, losses = Z(v, rows * V), Z(v, rows)
    v.call("softmax_crossentropy_soft_forward", probs, losses, D(v, z), D(v, ta, np.int32), D(v, tb, np.int32),
           0.3, 0.1, rows, 1, V)
    nan = np.isnan(losses.numpy())
    assert nan.tolist() == [False, False, True, False, False]
    assert np.all(np.isfinite(probs.numpy()))


@pytest.mark.parametrize("given_tb", [False, True])
@pytest.mark.parametrize("lam", [1.0, 0.3])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("rows,V", SHAPES)
def test_soft_backward_op(gpu, vit, rows, V, eps, lam, given_tb):
    v = gpu
    z, ta, tb = op_case(rows, V, given_tb)
    rng = np.random.default_rng(7)
    d0 = rng.normal(size=(rows, V)).astype(np.float32)
    dl = rng.uniform(0.1, 1.0, size=rows).astype(np.float32)
    z64 = z.astype(np.float64)
    p = np.exp(z64 - lse64(z64)[:, None])
    t = vit.mix.soft_targets(ta, tb, lam, eps, V)
    ref = d0.astype(np.float64) + (p - t) * dl.astype(np.float64)[:, None]
    gz = D(v, z)
    probs = Z(v, rows * V)
    v.call("softmax_forward", probs, gz, rows, 1, V)
    out = D(v, d0)
    v.call("crossentropy_soft_softmax_backward", out, D(v, dl), probs, D(v, ta, np.int32),
           D(v, tb, np.int32) if given_tb else None, lam, eps, rows, 1, V)
    bad, rep = parity.check({"dlogits": (out.numpy(), ref)}, parity.FP32)
    print(f"\nsoft bwd rows {rows} V {V} eps {eps} lam {lam}: {parity.summary(rep)}")
    assert not bad, bad
    # and the gradient alone (from zero), so the += start cannot hide it
    out0 = Z(v, rows * V)
    v.call("crossentropy_soft_softmax_backward", out0, D(v, dl), probs, D(v, ta, np.int32),
           D(v, tb, np.int32) if given_tb else None, lam, eps, rows, 1, V)
    bad, rep = parity.check({"dlogits0": (out0.numpy(), ref - d0)}, parity.FP32)
    assert not bad, bad


# ------------------------------------------------------------------ mix kernels
def boxes(img):
    return [(4, 4, 4, 9),                  # empty
            (7, 9, 8, 10),                 # one pixel
            (0, 0, img, img),              # the full image
            (3, 5, 10, 6),                 # [3,10) x [5,6): unaligned, one row
            (img - 9, img - 5, img, img)]  # touching the bottom-right corner


MIXES = [("mixup", 0.3), ("mixup", 0.0), ("mixup", 1.0)] + [("cutmix", k) for k in range(5)]


@pytest.mark.parametrize("kind,arg", MIXES)
@pytest.mark.parametrize("B", [4, 5])
@pytest.mark.parametrize("name", ["test", "test_t10"])
def test_mix_kernels_bit_identical_to_reference(gpu, vit, name, B, kind, arg):
    v = gpu
    cfg = v.data.CONFIGS[name]
    px, lab = v.data.synthetic_batch(cfg, B, seed=71)
    mode = v.MIX_MIXUP if kind == "mixup" else v.MIX_CUTMIX
    lam, box = (arg, None) if kind == "mixup" else (1.0, boxes(cfg.img)[arg])
    want, ta, tb, lam_used = vit.mix.reference_mix(px, lab, mode, lam, box)
    m = v.ViT(cfg, B, v.VIT_FP32)
    m.set_batch(px, lab)
    assert np.array_equal(m.pixels().view(np.uint32), px.view(np.uint32))
    m.mix_batch(mode, lam, box)
    got = m.pixels()
    m.close()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if B % 2:
        assert np.array_equal(got[B // 2].view(np.uint32), px[B // 2].view(np.uint32))
    if kind == "cutmix" and arg == 2:
        assert np.array_equal(got, px[::-1]) and lam_used == 0.0


@pytest.mark.parametrize("kind", ["mixup", "cutmix"])
def test_mix_after_set_batch_u8(gpu, vit, kind):
    """Mixing a batch that was normalised on the device (the uint8 staging path)."""
    v = gpu
    cfg = v.data.CONFIGS["test"]
    B = 5
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, size=(B, cfg.img, cfg.img, 3)).astype(np.uint8)
    lab = rng.integers(0, cfg.num_classes, size=B).astype(np.int32)
    m = v.ViT(cfg, B, v.VIT_FP32)
    m.set_batch_u8(img, lab)
    base = m.pixels()
    assert np.array_equal(base, v.data.normalize_u8(img, v.IMAGENET_MEAN, v.IMAGENET_STD))
    mode, lam, box = (v.MIX_MIXUP, 0.3, None) if kind == "mixup" else (v.MIX_CUTMIX, 1.0, (3, 5, 10, 20))
    want, _, _, _ = vit.mix.reference_mix(base, lab, mode, lam, box)
    m.mix_batch(mode, lam, box)
    got = m.pixels()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the next upload is unmixed again and can be mixed again
    m.set_batch_u8(img, lab)
    assert np.array_equal(m.pixels(), base)
    m.mix_batch(mode, lam, box)
    assert np.array_equal(m.pixels().view(np.uint32), want.view(np.uint32))
    m.close()


# ------------------------------------------------------------------ trainer vs the CPU oracle
def oracle_step(oc, o, cfg, params, px, lab, b_global=None):
    c = oc.VitConfig(cfg.img, cfg.patch, cfg.in_ch, cfg.channels, cfg.num_layers, cfg.num_heads,
                     cfg.num_classes)
    m = oc.RefViT(o, c, px.shape[0])
    p = o.arr(params)
    loss = m.forward(p, px, lab, b_global)
    g = np.zeros_like(p)
    m.backward(p, g)
    return loss, m.logits(), g


EPS = 0.1
TRAINER_MIXES = {"mixup": (1, 0.3, None), "cutmix": (2, 1.0, (8, 8, 24, 24))}


@functools.lru_cache(maxsize=None)
def soft_oracle(name, B, mix):
    """(params, px, lab, px', lam_used, hard pass on px', soft loss, logits, soft gradient) — the
    2 + V oracle passes, computed once per (config, batch, mix) and shared (never modified)."""
    import oracle_ctypes as oc
    from vitpkg import vit as v
    o = oc.Oracle("f32")
    cfg = v.data.CONFIGS[name]
    V = cfg.num_classes
    params = v.data.init_params(cfg, "parity", seed=3)
    px, lab = v.data.synthetic_batch(cfg, B, seed=5)
    mode, lam, box = TRAINER_MIXES[mix]
    pxm, ta, tb, lam_used = v.mix.reference_mix(px, lab, mode, lam, box)
    lam32 = np.float32(lam_used)
    oml = float(np.float32(1.0) - lam32)
    eps = float(np.float32(EPS))
    la, logits, ga = oracle_step(oc, o, cfg, params, pxm, ta)
    lb, _, gb = oracle_step(oc, o, cfg, params, pxm, tb)
    loss = (1 - eps) * (float(lam32) * la + oml * lb)
    g = (1 - eps) * (float(lam32) * ga.astype(np.float64) + oml * gb.astype(np.float64))
    for k in range(V):
        lk, _, gk = oracle_step(oc, o, cfg, params, pxm, np.full(B, k, np.int32))
        loss += eps / V * lk
        g += eps / V * gk.astype(np.float64)
    for a in (params, px, lab, pxm, logits, g, ga):
        a.setflags(write=False)
    return dict(cfg=cfg, params=params, px=px, lab=lab, pxm=pxm, lam=lam_used, hard=(la, ga),
                loss=float(loss), logits=logits, g=g)


def soft_run(v, r, B, prec, mix, eps=EPS):
    """One forward / backward of the trainer on the mixed, smoothed batch."""
    mode, lam, box = TRAINER_MIXES[mix]
    m = v.ViT.build(r["cfg"], B, prec, params=r["params"])
    m.set_label_smoothing(eps)
    m.set_batch(r["px"], r["lab"])
    m.mix_batch(mode, lam, box)
    m.zero_grad()
    loss = m.forward()
    m.backward()
    out = (loss, m.logits(), m.grads(), m.pixels())
    m.close()
    return out


def hard_run(v, r, B, prec):
    """The hard-label step on the same mixed pixels (the error the soft one is read next to)."""
    m = v.ViT.build(r["cfg"], B, prec, params=r["params"])
    m.zero_grad()
    loss = m.forward(r["pxm"], r["lab"])
    m.backward()
    out = (loss, m.logits(), m.grads())
    m.close()
    return out


def report(label, cfg, run, r, rule):
    loss, logits, g = run[:3]
    bad, rep = parity.check(parity.tensors(cfg, logits, g, r["logits"], r["g"].astype(np.float32)), rule)
    print(f"\n{label}: loss rel {abs(loss - r['loss']) / abs(r['loss']):.2e}; {parity.summary(rep)}")
    return bad, rep


@pytest.mark.parametrize("mix", ["mixup", "cutmix"])
def test_fp32_soft_trainer_vs_oracle(gpu, mix):
    v = gpu
    B = 5
    r = soft_oracle("test", B, mix)
    run = soft_run(v, r, B, v.VIT_FP32, mix)
    assert np.array_equal(run[3].view(np.uint32), r["pxm"].view(np.uint32))
    h = hard_run(v, r, B, v.VIT_FP32)
    _, hrep = parity.check(parity.tensors(r["cfg"], h[1], h[2], r["logits"], r["hard"][1]), parity.FP32)
    print(f"\nhard labels on the same pixels: loss rel {abs(h[0] - r['hard'][0]) / abs(r['hard'][0]):.2e}; "
          f"{parity.summary(hrep)}")
    bad, rep = report(f"fp32 test B={B} {mix} eps {EPS}", r["cfg"], run, r, parity.FP32)
    assert abs(run[0] - r["loss"]) <= 1e-4 * abs(r["loss"]), (run[0], r["loss"])
    assert not bad, bad


@functools.lru_cache(maxsize=None)
def bf16_pairs(mix):
    from vitpkg import vit as v
    r = soft_oracle("test_h64", 4, mix)
    run = soft_run(v, r, 4, v.VIT_BF16, mix)
    return run, parity.tensors(r["cfg"], run[1], run[2], r["logits"], r["g"].astype(np.float32))


@pytest.mark.parametrize("mix", ["mixup", "cutmix"])
def test_bf16_soft_trainer_vs_oracle(gpu, mix):
    v = gpu
    r = soft_oracle("test_h64", 4, mix)
    run, _ = bf16_pairs(mix)
    h = hard_run(v, r, 4, v.VIT_BF16)
    _, hrep = parity.check(parity.tensors(r["cfg"], h[1], h[2], r["logits"], r["hard"][1]), parity.BF16)
    print(f"\nhard labels on the same pixels: loss rel {abs(h[0] - r['hard'][0]) / abs(r['hard'][0]):.2e}; "
          f"{parity.summary(hrep)}")
    bad, rep = report(f"bf16 test_h64 B=4 {mix} eps {EPS}", r["cfg"], run, r, parity.BF16)
    assert abs(run[0] - r["loss"]) <= 1e-2 * abs(r["loss"]), (run[0], r["loss"])
    assert not bad, bad


@pytest.mark.parametrize("mix", ["mixup", "cutmix"])
def test_fp8_soft_trainer_vs_oracle(gpu, mix):
    v = gpu
    r = soft_oracle("test_h64", 4, mix)
    _, pb = bf16_pairs(mix)
    run = soft_run(v, r, 4, v.VIT_FP8, mix)
    pf = parity.tensors(r["cfg"], run[1], run[2], r["logits"], r["g"].astype(np.float32))
    rf = parity.fp8_report(pf)
    print(f"\nfp8 test_h64 B=4 {mix}: max tensor err {max(x['max'] for x in rf.values()):.3f}",
          {k: round(x["max"], 4) for k, x in rf.items()})
    bad = parity.check_fp8(pf, pb)
    assert not bad, bad


# ------------------------------------------------------------------ unused means unchanged
def three_steps(v, m, px, lab, mix=None):
    m.set_batch(px, lab)
    if mix is not None:
        m.mix_batch(*mix)
    m.sync()
    v.kernel_hits_reset()
    for _ in range(3):
        m.train_step(0.05)
    m.sync()
    hits = v.kernel_hits()
    return float(v.lib().vit_trainer_mean_loss(m.h)), m.grads(), m.params(), hits


@pytest.mark.parametrize("case", ["a_set_and_unset", "b_after_a_soft_step", "c_empty_box"])
@pytest.mark.parametrize("prec_name", ["VIT_BF16", "VIT_FP8"])
def test_unused_means_unchanged(gpu, prec_name, case):
    v = gpu
    prec = getattr(v, prec_name)
    cfg = v.data.CONFIGS["test_h64"]
    B = 4
    params = v.data.init_params(cfg, "parity", seed=33)
    px, lab = v.data.synthetic_batch(cfg, B, seed=34)
    fresh = v.ViT.build(cfg, B, prec, params=params)
    want = three_steps(v, fresh, px, lab)
    fresh.close()
    m = v.ViT.build(cfg, B, prec, params=params)
    mix = None
    if case == "a_set_and_unset":
        m.set_label_smoothing(0.1)
        m.set_label_smoothing(0.0)
        mix = (v.MIX_NONE,)
    elif case == "b_after_a_soft_step":
        px2, lab2 = v.data.synthetic_batch(cfg, B, seed=35)
        m.set_label_smoothing(0.1)
        m.set_batch(px2, lab2)
        m.mix_batch(v.MIX_MIXUP, 0.3)
        m.train_step(0.05)
        m.sync()
        m.set_label_smoothing(0.0)
        m.set_params(params)
    else:
        mix = (v.MIX_CUTMIX, 1.0, (5, 7, 5, 20))
    got = three_steps(v, m, px, lab, mix)
    m.close()
    assert got[0] == want[0]
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32))
    assert np.array_equal(got[3], want[3]), (np.nonzero(got[3] != want[3]), got[3], want[3])


# ------------------------------------------------------------------ determinism
@pytest.mark.parametrize("prec_name", ["VIT_BF16", "VIT_FP8"])
def test_mixed_smoothed_steps_are_bitwise_deterministic(gpu, prec_name):
    v = gpu
    prec = getattr(v, prec_name)
    cfg = v.data.CONFIGS["test_h64"]
    B = 8
    params = v.data.init_params(cfg, "parity", seed=23)
    px, lab = v.data.synthetic_batch(cfg, B, seed=24)
    mixes = [(v.MIX_MIXUP, 0.3, None), (v.MIX_CUTMIX, 1.0, (8, 8, 24, 24)), (v.MIX_MIXUP, 0.8, None)]
    runs = []
    for _ in range(2):
        m = v.ViT.build(cfg, B, prec, params=params)
        m.set_concurrency(True)
        m.set_label_smoothing(0.1)
        out = []
        for mix in mixes:
            m.set_batch(px, lab)
            m.mix_batch(*mix)
            m.train_step(0.05)
            m.sync()
            out.append((float(v.lib().vit_trainer_mean_loss(m.h)), m.grads(), m.params()))
        runs.append(out)
        m.close()
    for (l0, g0, p0), (l1, g1, p1) in zip(*runs):
        assert l0 == l1 and np.isfinite(l0)
        assert np.array_equal(g0.view(np.uint32), g1.view(np.uint32))
        assert np.array_equal(p0.view(np.uint32), p1.view(np.uint32))
    assert not np.array_equal(runs[0][0][2], params)


# ------------------------------------------------------------------ entropy floor
def test_smoothed_loss_falls_to_but_not_below_the_target_entropy(gpu, vit):
    """KL(t || p) >= 0: the soft-target loss can never be below H(t).  40 SGD steps on one smoothed
    batch: the loss falls, and stays above H(t) (1 - the fp32 loss tolerance)."""
    v = gpu
    cfg = v.data.CONFIGS["test"]
    B, eps = 5, 0.1
    params = v.data.init_params(cfg, "parity", seed=1)
    px, lab = v.data.synthetic_batch(cfg, B, seed=2)
    t = vit.mix.soft_targets(lab, None, 1.0, eps, cfg.num_classes)
    H = float(-(t * np.log(t)).sum(axis=1).mean())
    m = v.ViT.build(cfg, B, v.VIT_FP32, params=params)
    m.set_label_smoothing(eps)
    m.set_batch(px, lab)
    losses = []
    for _ in range(40):
        m.train_step(0.1)
        losses.append(float(v.lib().vit_trainer_mean_loss(m.h)))
    m.close()
    print(f"\nH(t) {H:.5f}; loss {losses[0]:.4f} -> {losses[-1]:.4f} (min {min(losses):.5f})")
    assert losses[-1] < losses[0], losses
    assert min(losses) >= H * (1 - parity.FP32["loss"]), (min(losses), H)


# ------------------------------------------------------------------ errors
def test_bad_arguments_are_errors_and_leave_the_batch_unmixed(gpu):
    v = gpu
    cfg = v.data.CONFIGS["test"]
    B = 4
    params = v.data.init_params(cfg, "parity", seed=1)
    px, lab = v.data.synthetic_batch(cfg, B, seed=2)
    m = v.ViT.build(cfg, B, v.VIT_FP32, params=params)
    loss0 = m.forward(px, lab)
    for eps in (1.0, -0.1):
        with pytest.raises(v.VitError, match="eps"):
            m.set_label_smoothing(eps)
    assert m.forward() == loss0  # smoothing still off
    img = cfg.img
    bad = [((v.MIX_MIXUP, 1.5, None), "lam"), ((v.MIX_MIXUP, -0.5, None), "lam"),
           ((v.MIX_MIXUP, float("nan"), None), "lam"),
           ((v.MIX_CUTMIX, 1.0, (0, 0, img + 1, 4)), "box"), ((v.MIX_CUTMIX, 1.0, (-1, 0, 4, 4)), "box"),
           ((v.MIX_CUTMIX, 1.0, (0, 8, 4, img + 8)), "box"), ((v.MIX_CUTMIX, 1.0, (9, 0, 4, 4)), "box"),
           ((3, 0.5, None), "mode"), ((-1, 0.5, None), "mode")]
    for args, word in bad:
        with pytest.raises(v.VitError, match=word):
            m.mix_batch(*args)
        assert np.array_equal(m.pixels(), px)
    assert m.forward() == loss0
    # a batch without labels cannot be mixed
    m.set_batch(px, None)
    with pytest.raises(v.VitError, match="labels"):
        m.mix_batch(v.MIX_MIXUP, 0.3)
    assert np.array_equal(m.pixels(), px)
    # none of the failures marked the batch: a first mix still works, a second one does not
    m.set_batch(px, lab)
    m.mix_batch(v.MIX_MIXUP, 0.3)
    once = m.pixels()
    assert not np.array_equal(once, px)
    for args in ((v.MIX_MIXUP, 0.3, None), (v.MIX_CUTMIX, 1.0, (0, 0, 4, 4))):
        with pytest.raises(v.VitError, match="already mixed"):
            m.mix_batch(*args)
    assert np.array_equal(m.pixels(), once)
    m.mix_batch(v.MIX_NONE)  # a no-op, always allowed
    m.set_batch(px, lab)      # the next batch is unmixed
    m.mix_batch(v.MIX_CUTMIX, 1.0, (0, 0, 4, 4))
    m.close()


def test_eval_counts_against_the_batch_own_labels(gpu):
    v = gpu
    cfg = v.data.CONFIGS["test"]
    B = 4
    params = v.data.init_params(cfg, "parity", seed=1)
    px, lab = v.data.synthetic_batch(cfg, B, seed=2)
    m = v.ViT.build(cfg, B, v.VIT_FP32, params=params)
    m.set_label_smoothing(0.1)
    m.set_batch(px, lab)
    m.mix_batch(v.MIX_MIXUP, 0.3)
    pred, correct = m.evaluate()
    m.close()
    assert correct == int((pred == lab).sum())
