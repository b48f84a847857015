"""EMA of the weights, host side (vit.rs_amd/ema.py, include/vit_checkpoint.h): the numpy
statement the kernels are compared with, the warm-up schedule, and the checkpoint layout with an EMA array.
No GPU."""
import ctypes
import os

import numpy as np
import pytest

F32 = np.float32
MAGIC, VERSION = 20261016, 1


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture
def cfg(vit):
    return vit.data.CONFIGS["test"]


def values(n, seed):
    """normal values with denormals, signed zeros and large magnitudes mixed in"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(n).astype(F32)
    special = np.array([0.0, -0.0, 1e-45, -3e-42, 1.1754942e-38, 1e-38, 3e38, -2.5e38, 65504.0, 1.0], F32)
    idx = rng.permutation(n)[:special.size]
    a[idx] = special[:idx.size]
    return a


# ------------------------------------------------------------------ ema_ref
@pytest.mark.parametrize("d", [0.5, 0.9, 0.999, 0.9999])
def test_ema_ref_is_the_stepwise_rounded_float64_statement(vit, d):
    e, p = values(4099, 1), values(4099, 2)
    got = vit.ema.ema_ref(e, p, d)
    # every operation exact in float64 (a product of two fp32 is; the sum of two fp32 rounds once more to
    # fp32 correctly: 53 >= 2 * 24 + 2), then rounded to fp32: three roundings, no fused step
    d32 = F32(d)
    omd = F32(1.0 - np.float64(d32))
    with np.errstate(over="ignore"):
        a = (np.float64(d32) * e.astype(np.float64)).astype(F32)
        b = (np.float64(omd) * p.astype(np.float64)).astype(F32)
        want = (a.astype(np.float64) + b.astype(np.float64)).astype(F32)
    assert got.dtype == np.float32
    assert np.array_equal(bits(got), bits(want))
    assert vit.ema.one_minus(d) == omd
    # the contracted form (the products kept exact into the sum) is a different function: the reference pins
    # the unfused one (at d = 0.5 both products are exact and the two agree)
    fused = (np.float64(d32) * e.astype(np.float64) + np.float64(omd) * p.astype(np.float64)).astype(F32)
    assert np.array_equal(bits(fused), bits(want)) == (d == 0.5)


def test_ema_ref_fixed_points(vit):
    x = values(1000, 3)
    x = x[(np.abs(x) < 1e30) & ((np.abs(x) > 1e-37) | (x == 0))]
    assert np.array_equal(bits(vit.ema.ema_ref(x, x, 0.5)), bits(x))  # 0.5 x + 0.5 x is exact for normal x
    z = np.zeros(8, F32)
    assert np.array_equal(bits(vit.ema.ema_ref(z, z, 0.9999)), bits(z))


def test_warmup_decay(vit):
    w = vit.ema.warmup_decay
    assert w(0.9999, 0) == pytest.approx(0.1)
    assert w(0.9999, 1) == pytest.approx(2.0 / 11.0)
    assert w(0.9999, 90) == pytest.approx(0.91)
    assert w(0.9, 90) == 0.9
    assert w(0.9999, 10 ** 7) == 0.9999
    prev = 0.0
    for u in range(200):
        assert prev <= w(0.9999, u) < 1.0
        prev = w(0.9999, u)


# ------------------------------------------------------------------ checkpoints
def arrays(cfg, seed=0):
    rng = np.random.default_rng(seed)
    n = cfg.num_params()
    p, m, v, e = (rng.standard_normal(n).astype(F32) for _ in range(4))
    return p, m, np.abs(v), e


HP = (0.9, 0.95, 1e-8, 0.1)


@pytest.mark.parametrize("opt", [False, True])
def test_round_trip_with_ema(vit, cfg, tmp_path, opt):
    p, m, v, e = arrays(cfg)
    n = cfg.num_params()
    path = tmp_path / "e.bin"
    updates = (1 << 33) + 5  # both halves of the count
    if opt:
        vit.write_checkpoint(path, cfg, p, m, v, step=7, adamw=HP, ema=e, ema_decay=0.9999, ema_updates=updates)
    else:
        vit.write_checkpoint(path, cfg, p, ema=e, ema_decay=0.9999, ema_updates=updates)
    raw = path.read_bytes()
    assert len(raw) == 1024 + 4 * n * ((3 if opt else 1) + 1)
    h = np.frombuffer(raw[:1024], np.int32)
    assert h[0] == MAGIC and h[1] == VERSION
    assert h[10] == (3 if opt else 2)
    assert h[18:19].view(np.float32)[0] == F32(0.9999)
    assert int(h[19:20].view(np.uint32)[0]) | (int(h[20:21].view(np.uint32)[0]) << 32) == updates
    assert not h[21:].any()
    body = np.frombuffer(raw[1024:], np.float32)
    assert np.array_equal(bits(body[:n]), bits(p)) and np.array_equal(bits(body[-n:]), bits(e))
    got, d, u = vit.read_checkpoint_ema(path, cfg)
    assert np.array_equal(bits(got), bits(e)) and d == float(F32(0.9999)) and u == updates
    # the functions from before the EMA read the same file and ignore the extra array
    info = vit.checkpoint_info(path)
    assert info["has_opt"] is opt and info["num_params"] == n and info["step"] == (7 if opt else 0)
    p2, m2, v2 = vit.read_checkpoint(path, cfg)
    assert np.array_equal(bits(p2), bits(p))
    if opt:
        assert np.array_equal(bits(m2), bits(m)) and np.array_equal(bits(v2), bits(v))
        assert np.allclose(info["adamw"], HP)
    else:
        assert m2 is None and v2 is None


@pytest.mark.parametrize("opt", [False, True])
def test_file_without_ema_has_the_bytes_of_the_old_call(vit, cfg, tmp_path, opt):
    p, m, v, e = arrays(cfg, 1)
    n = cfg.num_params()
    mv = (m, v) if opt else (None, None)
    a, b, c = tmp_path / "a.bin", tmp_path / "b.bin", tmp_path / "c.bin"
    vit.write_checkpoint(a, cfg, p, *mv, step=3, adamw=HP if opt else None)  # the wrapper, ema left out
    P = ctypes.c_void_p
    ptr = [x.ctypes.data_as(P) if x is not None else None for x in (p,) + mv]
    hp = vit.AdamWC(*HP)
    cc = vit._cfg_c(cfg)
    assert vit.lib().vit_checkpoint_write(os.fsencode(b), ctypes.byref(cc), *ptr, 3, ctypes.byref(hp) if opt else None) == 0
    assert vit.lib().vit_checkpoint_write_ex(os.fsencode(c), ctypes.byref(cc), *ptr, 3,
                                             ctypes.byref(hp) if opt else None, None, 0.75, 12) == 0
    # ... and the layout written out by hand, as it stood before the EMA fields existed
    h = np.zeros(256, np.int32)
    h[:14] = [MAGIC, VERSION, cfg.T, cfg.num_classes, cfg.num_layers, cfg.num_heads, cfg.channels, cfg.img, cfg.patch,
              cfg.in_ch, int(opt), 3 if opt else 0, n, 0]
    if opt:
        h[14:18] = np.array(HP, F32).view(np.int32)
    want = h.tobytes() + p.tobytes() + (m.tobytes() + v.tobytes() if opt else b"")
    assert a.read_bytes() == want
    assert b.read_bytes() == want
    assert c.read_bytes() == want
    assert vit.read_checkpoint_ema(a, cfg) == (None, 0.0, 0)


def test_truncated_or_padded_ema_file_is_rejected(vit, cfg, tmp_path):
    p, m, v, e = arrays(cfg, 2)
    path = tmp_path / "t.bin"
    vit.write_checkpoint(path, cfg, p, m, v, step=1, adamw=HP, ema=e, ema_decay=0.99, ema_updates=4)
    raw = path.read_bytes()
    n = cfg.num_params()
    for cut in (raw[:-4], raw[:-4 * n], raw + b"\0\0\0\0"):  # (the second: the flag says EMA, the array is gone)
        bad = tmp_path / "bad.bin"
        bad.write_bytes(cut)
        with pytest.raises(vit.VitError):
            vit.checkpoint_info(bad)
        with pytest.raises(vit.VitError):
            vit.read_checkpoint_ema(bad, cfg)
        with pytest.raises(vit.VitError):
            vit.read_checkpoint(bad, cfg)
    other = vit.data.CONFIGS["test_h64"]
    with pytest.raises(vit.VitError):
        vit.read_checkpoint_ema(path, other)
    with pytest.raises(vit.VitError):  # a negative update count
        vit.write_checkpoint(tmp_path / "n.bin", cfg, p, ema=e, ema_decay=0.9, ema_updates=-1)


def test_symbols_and_wrappers(vit):
    names = vit.exported_symbols()
    for s in ("vit_trainer_set_ema", "vit_trainer_get_ema", "vit_trainer_set_ema_params", "vit_trainer_get_ema_info",
              "vit_trainer_ema_weights", "ema_update", "vit_checkpoint_write_ex", "vit_checkpoint_read_ema"):
        assert s in names, s
        assert hasattr(vit.lib(), s), s
    for meth in ("set_ema", "ema", "set_ema_params", "ema_info", "ema_weights"):
        assert callable(getattr(vit.ViT, meth)), meth
    assert vit.HIT_EMA < len(vit.kernel_hits())
    # the declarations are in the public headers
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(vit.__file__))), "include")
    text = "".join(open(os.path.join(inc, f)).read() for f in ("vit_trainer.h", "vit_ops.h", "vit_checkpoint.h"))
    for s in names:
        if "ema" in s:
            assert s + "(" in text, s
