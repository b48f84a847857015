"""The LAMB reference (tests/lamb_ref.py) against the CPU oracle's AdamW and a float64 restatement of timm's
Lamb step; its flag and branch logic.  No GPU."""
import numpy as np
import pytest

import lamb_ref as lr_

F32 = np.float32
HP = dict(beta1=0.9, beta2=0.95, eps=1e-6)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def tensors(n, seed, dt=F32):
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal(n) * 0.05).astype(dt)
    g = (rng.standard_normal(n) * 1e-3).astype(dt)
    m = (rng.standard_normal(n) * 1e-3).astype(dt)
    v = (rng.standard_normal(n) ** 2 * 1e-6).astype(dt)
    return p, g, m, v


@pytest.mark.parametrize("t", [1, 2, 7])
@pytest.mark.parametrize("wd", [0.0, 0.05])
def test_moments_are_the_oracles(oracle32, t, wd):
    """lr = 0: the oracle leaves p alone and advances m, v"""
    o = oracle32
    p, g, m, v = tensors(1000, 1 + t)
    out = lr_.lamb_segment(p, g, m, v, 1e-3, wd_e=wd, t=t, **HP)
    po, mo, vo = o.arr(p.copy()), o.arr(m.copy()), o.arr(v.copy())
    o.adamw_step(po, o.arr(g), mo, vo, 0.0, HP["beta1"], HP["beta2"], HP["eps"], wd, t)
    assert np.array_equal(bits(out["m"]), bits(mo)) and np.array_equal(bits(out["v"]), bits(vo))
    # (p - 0 * u == p unless u is not finite)
    assert np.array_equal(bits(po), bits(p))


@pytest.mark.parametrize("t", [1, 3])
@pytest.mark.parametrize("wd", [0.0, 0.05])
def test_ratio_one_is_adamw(oracle32, t, wd):
    o = oracle32
    p, g, m, v = tensors(1537, 10 + t)
    out = lr_.lamb_segment(p, g, m, v, 3e-3, wd_e=wd, t=t, r=F32(1), **HP)
    po, mo, vo = o.arr(p.copy()), o.arr(m.copy()), o.arr(v.copy())
    o.adamw_step(po, o.arr(g), mo, vo, 3e-3, HP["beta1"], HP["beta2"], HP["eps"], wd, t)
    assert np.array_equal(bits(out["p"]), bits(po))
    assert not np.array_equal(bits(po), bits(p))
    if wd:  # ... and the ratio the reference computes itself does change the step
        own = lr_.lamb_segment(p, g, m, v, 3e-3, wd_e=wd, t=t, **HP)
        assert own["r"] != 1 and not np.array_equal(bits(own["p"]), bits(po))


def timm_lamb_step(p, g, m, v, lr, beta1, beta2, eps, wd, t, always_adapt, trust_clip):
    """timm.optim.Lamb.step for one parameter, grad_averaging on, max_grad_norm off, bias correction on,
    restated on float64 torch tensors -> (p', m', v')"""
    import math

    import torch
    p, g, m, v = (torch.from_numpy(a.copy()) for a in (p, g, m, v))
    one = torch.tensor(1.0, dtype=torch.float64)
    bc1, bc2 = 1 - beta1 ** t, 1 - beta2 ** t
    m.mul_(beta1).add_(g, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    denom = (v.sqrt() / math.sqrt(bc2)).add_(eps)
    update = (m / bc1).div_(denom)
    if wd != 0:
        update.add_(p, alpha=wd)
    if wd != 0 or always_adapt:
        w_norm, g_norm = p.norm(2.0), update.norm(2.0)
        trust = torch.where(w_norm > 0, torch.where(g_norm > 0, w_norm / g_norm, one), one)
        if trust_clip:
            trust = torch.minimum(trust, one)
        update.mul_(trust)
    p.add_(update, alpha=-lr)
    return p.numpy(), m.numpy(), v.numpy()


@pytest.mark.parametrize("always_adapt, trust_clip", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("wd", [0.0, 0.02])
@pytest.mark.parametrize("scale", [1e3, 1e-2])  # ratios above and below 1
def test_float64_agrees_with_timm(wd, always_adapt, trust_clip, scale):
    f64 = np.float64
    p, g, m, v = tensors(4099, 21, f64)
    p = p * scale
    flags = (lr_.ALWAYS_ADAPT if always_adapt else 0) | (lr_.TRUST_CLIP if trust_clip else 0)
    for t in (1, 2, 5):
        out = lr_.lamb_segment(p, g, m, v, 2e-3, wd_e=wd, t=t, flags=flags, dt=f64, **HP)
        want = timm_lamb_step(p, g, m, v, 2e-3, HP["beta1"], HP["beta2"], HP["eps"], wd, t, always_adapt, trust_clip)
        for got, ref in zip((out["p"], out["m"], out["v"]), want):
            err = np.abs(got - ref).max() / np.abs(ref).max()
            assert err <= 1e-12, (t, err)
        p, m, v = out["p"], out["m"], out["v"]
        g = g * 0.9


def test_branches():
    n = 300
    p, g, m, v = tensors(n, 31)
    z = np.zeros(n, F32)
    # a zero tensor: wn = 0 -> r = 1
    out = lr_.lamb_segment(z, g, m, v, 1e-3, wd_e=0.1, t=1, flags=lr_.ALWAYS_ADAPT, **HP)
    assert out["wn"] == 0 and out["un"] > 0 and out["r"] == 1
    # a zero direction: un = 0 -> r = 1
    out = lr_.lamb_segment(p, z, z, z, 1e-3, wd_e=0.0, t=1, flags=lr_.ALWAYS_ADAPT, **HP)
    assert out["wn"] > 0 and out["un"] == 0 and out["r"] == 1
    assert np.array_equal(bits(out["p"]), bits(p))
    # wd = 0: adapted only under the flag
    a = lr_.lamb_segment(p, g, m, v, 1e-3, wd_e=0.0, t=1, **HP)
    b = lr_.lamb_segment(p, g, m, v, 1e-3, wd_e=0.0, t=1, flags=lr_.ALWAYS_ADAPT, **HP)
    assert a["r"] == 1 and b["r"] == F32(b["wn"]) / F32(b["un"]) and b["r"] != 1
    assert a["wn"] == b["wn"] and a["un"] == b["un"]
    # trust_clip: a ratio above 1 becomes 1, one below 1 stays
    big = lr_.lamb_segment(p * F32(1e4), g, m, v, 1e-3, wd_e=0.01, t=1, **HP)
    assert big["r"] > 1
    assert lr_.lamb_segment(p * F32(1e4), g, m, v, 1e-3, wd_e=0.01, t=1, flags=lr_.TRUST_CLIP, **HP)["r"] == 1
    small = lr_.lamb_segment(p * F32(1e-4), g, m, v, 1e-3, wd_e=0.01, t=1, **HP)
    assert 0 < small["r"] < 1
    assert lr_.lamb_segment(p * F32(1e-4), g, m, v, 1e-3, wd_e=0.01, t=1, flags=lr_.TRUST_CLIP,
                            **HP)["r"] == small["r"]
    # NaN norms fall to 1
    assert lr_.ratio(F32(np.nan), F32(1), 0.1, 0) == 1 and lr_.ratio(F32(1), F32(np.nan), 0.1, lr_.TRUST_CLIP) == 1


def test_package_exports_lamb(vit):
    """the ctypes table and the wrapper carry the new entry points (the library itself: the GPU tests)"""
    for name in ("vit_trainer_step_lamb", "vit_trainer_get_lamb_info", "lamb_step"):
        assert name in vit.exported_symbols()
    assert vit.lamb_flags(True, True) == 3 and vit.lamb_flags() == 0
    assert hasattr(vit.ViT, "optimizer_step_lamb") and hasattr(vit.ViT, "lamb_info")
