"""Stochastic depth, host side (no GPU): vit_drop_path_draw against its Python statement, and the
reference step of tests/droppath_ref.py pinned against the oracle's own model (all-ones scales, bit
for bit) and against fp64 central finite differences (a table mixing 0, 1.25 and 2)."""
import ctypes
import os

import numpy as np
import pytest

import droppath_ref
from conftest import ROOT
from test_oracle import _fd_check

GOLDEN = os.path.join(ROOT, "tests", "golden")


# ------------------------------------------------------------------ the draw
@pytest.mark.parametrize("linear", [0, 1])
@pytest.mark.parametrize("L", [1, 2, 12])
@pytest.mark.parametrize("rate", [0.1, 0.3, 0.5])
def test_draw_matches_python_statement(vit, linear, L, rate):
    dp = vit.droppath
    B = 7
    for seed, key in ((1337, 0), (1337, 5), (2 ** 63 + 11, 3 * 8 + 1)):
        got = dp.draw(seed, key, L, B, rate, bool(linear))
        ref = dp.reference_draw(seed, key, L, B, rate, bool(linear))
        assert got.dtype == np.float32 and got.shape == (L, 2, B)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (seed, key)
        # every entry is 0 or the fp32 quotient 1 / (1 - p_l) of its layer
        p = dp.rates(L, rate, bool(linear))
        for l in range(L):
            keep = np.float32(1.0) / (np.float32(1.0) - p[l])
            assert set(np.unique(got[l])) <= {np.float32(0.0), keep}
    if linear and L > 1:
        assert np.all(dp.draw(1, 2, L, B, rate, True)[0] == 1.0)  # p_0 = 0: layer 0 is never dropped


def test_draw_drops_about_rate(vit):
    tab = vit.droppath.draw(7, 1, 2, 4096, 0.25, False)
    frac = float(np.mean(tab == 0.0))
    assert abs(frac - 0.25) < 0.02, frac  # 16384 draws: sigma 0.0034
    assert not np.array_equal(tab, vit.droppath.draw(7, 2, 2, 4096, 0.25, False))  # another key, another mask


@pytest.mark.parametrize("linear", [0, 1])
@pytest.mark.parametrize("L", [1, 2, 12])
def test_draw_rate_zero_is_all_ones(vit, linear, L):
    tab = vit.droppath.draw(3, 9, L, 5, 0.0, bool(linear))
    assert np.array_equal(tab, np.ones((L, 2, 5), np.float32))


@pytest.mark.parametrize("rate", [1.0, 1.5, -0.1, float("nan"), float("inf")])
def test_draw_rejects_bad_rate(vit, rate):
    L = vit.lib()
    out = np.full(2 * 2 * 3, -7.0, np.float32)
    rc = L.vit_drop_path_draw(1, 1, 2, 3, rate, 1, out.ctypes.data_as(ctypes.c_void_p))
    assert rc != 0
    msg = ctypes.c_char_p()
    assert L.vit_last_error(ctypes.byref(msg)) and b"vit_drop_path_draw" in msg.value
    L.vit_clear_error()
    assert np.all(out == -7.0)


def test_python_surface(vit):
    for name in ("vit_drop_path_draw", "vit_trainer_set_drop_path", "vit_trainer_get_drop_path",
                 "gemm_bf16_fused_rowscale"):
        assert name in vit.exported_symbols()
    assert hasattr(vit.ViT, "set_drop_path") and hasattr(vit.ViT, "drop_path")
    assert hasattr(vit.droppath, "DropPath")


def test_helper_keys_by_step_and_rank(vit):
    class Fake:
        B = 4
        cfg = vit.data.CONFIGS["test"]
        tab = None

        def set_drop_path(self, t):
            self.tab = t

    h = vit.droppath.DropPath(0.5, linear=False, seed=11)
    m = Fake()
    t = h.apply(m, step=3, rank=1, world=2)
    assert np.array_equal(t, vit.droppath.draw(11, 7, 2, 4, 0.5, False)) and m.tab is t
    assert vit.droppath.DropPath(0.0).apply(m, 0) is None


# ------------------------------------------------------------------ the reference step
def _golden(vit):
    z = np.load(os.path.join(GOLDEN, "test.npz"))
    return vit.data.CONFIGS["test"], z["params"], z["pixels"], z["labels"]


def test_reference_all_ones_is_refvit_bitwise(vit, oracle32):
    from test_gpu_model import oracle_step
    import oracle_ctypes as oc
    cfg, params, px, lab = _golden(vit)
    loss_r, logits_r, g_r = oracle_step(oc, oracle32, cfg, params, px, lab)
    for scales in (None, np.ones((cfg.num_layers, 2, px.shape[0]), np.float32)):
        loss, logits, g = droppath_ref.step(oracle32, cfg, params, px, lab, scales)
        assert np.float32(loss).tobytes() == np.float32(loss_r).tobytes(), (loss, loss_r)
        assert np.array_equal(logits.view(np.uint32), logits_r.view(np.uint32))
        for (name, a), b in zip(cfg.split(g).items(), cfg.split(g_r).values()):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name


def test_reference_finite_differences(vit, oracle64):
    o = oracle64
    cfg, params, px, lab = _golden(vit)
    B = px.shape[0]
    scales = np.array([[[0.0, 1.25], [2.0, 1.0]], [[1.25, 2.0], [1.0, 0.0]]])  # [L=2][2][B=2]
    assert scales.shape == (cfg.num_layers, 2, B)
    p = o.arr(params)
    _, _, g = droppath_ref.step(o, cfg, p, px, lab, scales)

    def loss():
        return droppath_ref.step(o, cfg, p, px, lab, scales, backward=False)[0]

    off = 0
    for k, (name, t) in enumerate(cfg.split(g).items()):
        _fd_check(o, loss, p[off:off + t.size], g[off:off + t.size], n_probe=12, seed=k)
        off += t.size
    assert off == p.size
    # a dropped branch's parameters get no gradient from the image it was dropped for, and the step
    # differs from the table-free one
    _, _, g1 = droppath_ref.step(o, cfg, p, px, lab, None)
    assert not np.allclose(g, g1)
