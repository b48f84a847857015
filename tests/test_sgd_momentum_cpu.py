"""Momentum SGD, host side (vit.rs_amd/sgd.py, include/vit_checkpoint.h): the numpy statement
the kernels are compared with against torch.optim.SGD in float64, and the checkpoint layout with a momentum
buffer.  No GPU."""
import ctypes
import itertools
import os

import numpy as np
import pytest

F32 = np.float32
MAGIC, VERSION = 20261016, 1
HP = (0.9, 0.95, 1e-8, 0.1)
SGD = (0.9, 0.0, 5e-4, True)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture
def cfg(vit):
    return vit.data.CONFIGS["test"]


# ------------------------------------------------------------------ sgd_ref against torch
# (momentum, dampening, weight decay, nesterov)
SETTINGS = [(0.9, 0.0, 0.0, False), (0.9, 0.0, 0.0, True), (0.9, 0.1, 5e-4, False), (0.9, 0.0, 5e-4, True),
            (0.5, 0.5, 0.0, False)]


@pytest.mark.parametrize("mu,damp,wd,nesterov", SETTINGS)
def test_sgd_ref_is_torch_sgd_in_float64(vit, mu, damp, wd, nesterov):
    """6 steps, n = 4099, lr 0.05: the decay order (coupled, in front of the buffer), the first-step buffer
    (buf = grad, no dampening), dampening and the Nesterov form are torch's.  In float64 both evaluate the same
    expression up to a contraction in torch's kernels: the max-normalised difference stays at a few ulp of
    float64 (2.2e-16); the bound 1e-13 leaves room for another libm or torch build and nothing more."""
    import torch
    n, lr, steps = 4099, 0.05, 6
    rng = np.random.default_rng(11)
    p0 = rng.standard_normal(n)
    grads = [rng.standard_normal(n) for _ in range(steps)]
    tp = torch.nn.Parameter(torch.tensor(p0, dtype=torch.float64))
    opt = torch.optim.SGD([tp], lr=lr, momentum=mu, dampening=damp, weight_decay=wd, nesterov=nesterov)
    p, b = p0.copy(), None
    worst = 0.0
    for k, g in enumerate(grads):
        tp.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        p, b = vit.sgd.sgd_ref(p, g, b, k == 0, lr, mu, damp, wd, nesterov, dtype=np.float64)
        assert p.dtype == np.float64 and b.dtype == np.float64
        want_p = tp.detach().numpy()
        want_b = opt.state[tp]["momentum_buffer"].numpy()
        for got, want in ((p, want_p), (b, want_b)):
            worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
    print(f"sgd_ref vs torch.optim.SGD float64 {(mu, damp, wd, nesterov)}: max-normalised difference {worst:.3g}")
    assert worst <= 1e-13, worst
    assert not np.array_equal(p, p0)


def test_sgd_ref_fp32_statement(vit):
    """the fp32 form is the float64 statement rounded after every operation (a product of two fp32 is exact in
    float64 and a sum of two fp32 rounds correctly through it), signed zeros of a first step included"""
    n = 1031
    rng = np.random.default_rng(5)
    p, g, b = (rng.standard_normal(n).astype(F32) for _ in range(3))
    g[:4] = [0.0, -0.0, 1e-45, -3e-42]
    lr, mu, damp, wd = F32(0.05), F32(0.9), F32(0.1), F32(5e-4)
    omd = F32(1.0 - np.float64(damp))
    assert vit.sgd.one_minus(damp) == omd
    D = np.float64

    def r(x):
        return x.astype(F32)

    for first, nesterov, c in itertools.product((True, False), (False, True), (None, 0.37)):
        got_p, got_b = vit.sgd.sgd_ref(p, g, b, first, lr, mu, 0.0 if nesterov else damp, wd, nesterov, c=c)
        o = F32(1.0) if nesterov else omd
        g1 = g if c is None else r(D(F32(c)) * g.astype(D))
        g2 = r(g1.astype(D) + r(D(wd) * p.astype(D)).astype(D))
        bn = g2 if first else r(r(D(mu) * b.astype(D)).astype(D) + r(D(o) * g2.astype(D)).astype(D))
        d = r(g2.astype(D) + r(D(mu) * bn.astype(D)).astype(D)) if nesterov else bn
        want_p = r(p.astype(D) - r(D(lr) * d.astype(D)).astype(D))
        assert got_p.dtype == np.float32 and got_b.dtype == np.float32
        assert np.array_equal(bits(got_p), bits(want_p)) and np.array_equal(bits(got_b), bits(bn))
    # weight decay 0 skips the term: a first step's buffer has the gradient's bits, -0 included
    _, b0 = vit.sgd.sgd_ref(p, g, None, True, lr, mu, 0.0, 0.0, False)
    assert np.array_equal(bits(b0), bits(g))
    # lr = 0 keeps the values and still advances the buffer
    p1, b1 = vit.sgd.sgd_ref(p, g, b, False, 0.0, mu, damp, wd, False)
    assert np.array_equal(bits(p1), bits(p)) and not np.array_equal(bits(b1), bits(b))


def test_presets(vit):
    assert vit.sgd.preset("momentum") == dict(momentum=0.9, dampening=0.0, nesterov=False, weight_decay=0.0)
    assert vit.sgd.preset("sgd", 5e-5) == dict(momentum=0.9, dampening=0.0, nesterov=True, weight_decay=5e-5)
    with pytest.raises(ValueError):
        vit.sgd.preset("adam")


# ------------------------------------------------------------------ checkpoints
def arrays(cfg, seed=0):
    rng = np.random.default_rng(seed)
    n = cfg.num_params()
    p, m, v, e, b = (rng.standard_normal(n).astype(F32) for _ in range(5))
    return p, m, np.abs(v), e, b


def write(vit, path, cfg, arrs, opt, ema, mom, steps=5):
    p, m, v, e, b = arrs
    kw = {}
    if opt:
        kw.update(m=m, v=v, step=7, adamw=HP)
    if ema:
        kw.update(ema=e, ema_decay=0.9999, ema_updates=9)
    if mom:
        kw.update(momentum=b, sgd=SGD, momentum_steps=steps)
    vit.write_checkpoint(path, cfg, p, **kw)


@pytest.mark.parametrize("opt,ema,mom", list(itertools.product((False, True), repeat=3)))
def test_all_eight_layouts(vit, cfg, tmp_path, opt, ema, mom):
    """read_info accepts every combination of (AdamW, EMA, momentum); each section comes back from its own
    reader, and an older layout is a prefix of the one with the momentum buffer behind it"""
    arrs = arrays(cfg)
    p, m, v, e, b = arrs
    n = cfg.num_params()
    path = tmp_path / "x.bin"
    steps = (1 << 33) + 3  # both halves of the count
    write(vit, path, cfg, arrs, opt, ema, mom, steps)
    raw = path.read_bytes()
    assert len(raw) == 1024 + 4 * n * (1 + 2 * opt + ema + mom)
    h = np.frombuffer(raw[:1024], np.int32)
    assert h[0] == MAGIC and h[1] == VERSION and h[10] == (opt | ema << 1 | mom << 2)
    info = vit.checkpoint_info(path)
    assert info["has_opt"] is opt and info["num_params"] == n
    p2, m2, v2 = vit.read_checkpoint(path, cfg)
    assert np.array_equal(bits(p2), bits(p))
    assert (m2 is None) == (not opt) and (not opt or (np.array_equal(bits(m2), bits(m)) and np.array_equal(bits(v2), bits(v))))
    e2, d2, u2 = vit.read_checkpoint_ema(path, cfg)
    assert (e2 is None) == (not ema) and (not ema or (np.array_equal(bits(e2), bits(e)) and u2 == 9))
    b2, sg, st = vit.read_checkpoint_momentum(path, cfg)
    if mom:
        assert np.array_equal(bits(b2), bits(b)) and st == steps
        assert sg == (float(F32(0.9)), 0.0, float(F32(5e-4)), True)
        assert int(h[21:22].view(np.uint32)[0]) | (int(h[22:23].view(np.uint32)[0]) << 32) == steps
        assert np.array_equal(h[23:26].view(np.float32), np.array(SGD[:3], F32)) and h[26] == 1
        assert not h[27:].any()
        assert np.array_equal(bits(np.frombuffer(raw[-4 * n:], np.float32)), bits(b))  # the last array
        # the file without the section is a prefix, up to the header fields of the section
        write(vit, tmp_path / "y.bin", cfg, arrs, opt, ema, False)
        old = (tmp_path / "y.bin").read_bytes()
        assert raw[1024:len(old)] == old[1024:]
        ho = np.frombuffer(old[:1024], np.int32).copy()
        assert not ho[21:].any()
        ho[10] |= 4
        ho[21:27] = h[21:27]
        assert ho.tobytes() == raw[:1024]
    else:
        assert (b2, sg, st) == (None, (0.0, 0.0, 0.0, False), 0)
        assert not h[21:].any()


@pytest.mark.parametrize("opt,ema", list(itertools.product((False, True), repeat=2)))
def test_null_buffer_writes_the_bytes_of_write_ex(vit, cfg, tmp_path, opt, ema):
    p, m, v, e, b = arrays(cfg, 1)
    P = ctypes.c_void_p
    ptr = [x.ctypes.data_as(P) if x is not None else None for x in ((p, m, v) if opt else (p, None, None))]
    hp = vit.AdamWC(*HP)
    sg = vit.SgdC(*SGD)
    cc = vit._cfg_c(cfg)
    ep = e.ctypes.data_as(P) if ema else None
    a, c = tmp_path / "a.bin", tmp_path / "c.bin"
    assert vit.lib().vit_checkpoint_write_ex(os.fsencode(a), ctypes.byref(cc), *ptr, 3, ctypes.byref(hp) if opt else None,
                                             ep, 0.75, 12) == 0
    # (the setting and the count are ignored with a NULL buffer)
    assert vit.lib().vit_checkpoint_write_sgd(os.fsencode(c), ctypes.byref(cc), *ptr, 3,
                                              ctypes.byref(hp) if opt else None, ep, 0.75, 12, None, ctypes.byref(sg),
                                              77) == 0
    assert a.read_bytes() == c.read_bytes()
    assert vit.read_checkpoint_momentum(c, cfg) == (None, (0.0, 0.0, 0.0, False), 0)


def test_truncated_momentum_file_is_rejected(vit, cfg, tmp_path):
    arrs = arrays(cfg, 2)
    path = tmp_path / "t.bin"
    write(vit, path, cfg, arrs, True, True, True)
    raw = path.read_bytes()
    n = cfg.num_params()
    for cut in (raw[:-4], raw[:-4 * n], raw + b"\0\0\0\0"):  # (the second: the flag says momentum, the array is gone)
        bad = tmp_path / "bad.bin"
        bad.write_bytes(cut)
        with pytest.raises(vit.VitError):
            vit.checkpoint_info(bad)
        with pytest.raises(vit.VitError):
            vit.read_checkpoint_momentum(bad, cfg)
        with pytest.raises(vit.VitError):
            vit.read_checkpoint(bad, cfg)
    with pytest.raises(vit.VitError):
        vit.read_checkpoint_momentum(path, vit.data.CONFIGS["test_h64"])
    with pytest.raises(vit.VitError):  # a negative step count
        vit.write_checkpoint(tmp_path / "n.bin", cfg, arrs[0], momentum=arrs[4], sgd=SGD, momentum_steps=-1)


def test_symbols_and_wrappers(vit):
    names = vit.exported_symbols()
    for s in ("vit_trainer_set_sgd", "vit_trainer_get_sgd_info", "vit_trainer_get_momentum", "sgd_momentum_step",
              "vit_checkpoint_write_sgd", "vit_checkpoint_read_momentum"):
        assert s in names, s
        assert hasattr(vit.lib(), s), s
    for meth in ("set_sgd", "sgd_info", "momentum"):
        assert callable(getattr(vit.ViT, meth)), meth
    assert callable(vit.sgd_momentum_step) and callable(vit.read_checkpoint_momentum)
    assert vit.HIT_SGDM == 97 and vit.HIT_SGDM < len(vit.kernel_hits())
