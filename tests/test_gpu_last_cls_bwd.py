"""Option last_cls_bwd: with last_cls on, the gradients entering the last block are zero
off the CLS rows, so its three weight gradients walk only the K-steps of the token axis that hold a CLS
row (1), and its fcproj input gradient runs on the CLS rows alone, storing each row's products into the
fc-bias partial row the full-size call summed it into (2).  Every skipped product is an exact zero
added to a +0 accumulator, so every check here is bit for bit against last_cls_bwd=0.

Geometry of tests/test_gpu_last_cls.py (C = 256, 4 heads, 2 layers, 224^2 / 16, T = 197).  B = 32 is
the smallest batch whose token count 32 x 197 is a multiple of the 256x128 engine's 32-row K-step, so
the weight gradients reach it; with two micro-batch streams its micro-batches have 16 x 197 rows.
B = 64 is the launch-mix shape.  B = 8 (1576 tokens) never reaches that engine: the option must leave
the step as it is.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _cfg(v):
    return v.data.VitCfg("prod_l2", img=224, patch=16, channels=256, num_layers=2, num_heads=4, num_classes=1000)


_inputs_cache = {}
_ref_cache = {}


def _inputs(v, cfg, B, seed=5):
    key = (cfg.name, B, seed)
    if key not in _inputs_cache:
        params = v.data.init_params(cfg, "parity", seed=3)
        px, lab = v.data.synthetic_batch(cfg, B, seed=seed)
        _inputs_cache[key] = (params, px, lab)
    return _inputs_cache[key]


def _trainer(v, cfg, B, prec, nmb, bwd, params, last_cls=1):
    m = v.ViT.build(cfg, B, prec, params=params)
    m.set_concurrency(True)
    m.set_option("microbatch", nmb)
    m.set_option("last_cls", last_cls)
    m.set_option("last_cls_bwd", bwd)
    return m


def _fwd_bwd(m, px, lab):
    m.set_batch(px, lab)
    m.zero_grad()
    loss = m.forward()
    m.backward()
    return loss, m.logits().copy(), m.grads()


def _run(v, cfg, B, prec, nmb, bwd, seed=5):
    """(loss, logits, grads) after one forward / backward and (logits, params) after three train_steps,
    each on a fresh trainer."""
    params, px, lab = _inputs(v, cfg, B, seed)
    m = _trainer(v, cfg, B, prec, nmb, bwd, params)
    one = _fwd_bwd(m, px, lab)
    m.close()
    m = _trainer(v, cfg, B, prec, nmb, bwd, params)
    m.set_batch(px, lab)
    for _ in range(3):
        m.train_step(0.05)
    m.sync()
    three = (m.logits().copy(), m.params())
    m.close()
    return one, three


def _ref(v, cfg, B, prec, nmb):
    key = (cfg.name, B, prec, nmb)
    if key not in _ref_cache:
        _ref_cache[key] = _run(v, cfg, B, prec, nmb, 0)
    return _ref_cache[key]


def _same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), \
        (what, int(np.sum(a.view(np.uint32) != b.view(np.uint32))))


def _compare(cfg, got, want):
    (l1, z1, g1), (z3, p3) = got
    (l0, z0, g0), (y3, q3) = want
    assert np.isfinite(l1) and np.isfinite(g1).all() and np.isfinite(p3).all()
    assert np.float32(l1).tobytes() == np.float32(l0).tobytes(), (l1, l0)
    _same_bits(z1, z0, "logits")
    t1, t0 = cfg.split(g1), cfg.split(g0)
    assert len(t1) == 20
    for name in t1:
        _same_bits(t1[name], t0[name], name)
    _same_bits(z3, y3, "logits after 3 steps")
    _same_bits(p3, q3, "params after 3 steps")


@pytest.mark.parametrize("bwd", [1, 2])
@pytest.mark.parametrize("B,nmb", [(32, 1), (32, 2), (64, 1), (64, 2), (8, 1), (8, 2)])
def test_on_equals_off(gpu, B, nmb, bwd):
    """Loss, logits and all 20 gradient tensors after one forward / backward, and logits and parameters
    after three train_steps, against last_cls_bwd=0."""
    v = gpu
    cfg = _cfg(v)
    _compare(cfg, _run(v, cfg, B, v.VIT_BF16, nmb, bwd), _ref(v, cfg, B, v.VIT_BF16, nmb))


@pytest.mark.parametrize("nmb", [1, 2])
@pytest.mark.parametrize("first", ["last_cls=0", "last_cls_bwd=0"])
def test_no_stale_rows_leak(gpu, nmb, first):
    """A step on batch 1 with last_cls off (every buffer then holds real non-CLS rows) or with
    last_cls_bwd off (dfch and the fc-bias partial rows hold a full-size step's), then last_cls_bwd=2 on
    batch 2: the bits of a fresh trainer that saw only batch 2."""
    v = gpu
    cfg = _cfg(v)
    B = 32
    params, px1, lab1 = _inputs(v, cfg, B, seed=5)
    _, px2, lab2 = _inputs(v, cfg, B, seed=11)
    m = _trainer(v, cfg, B, v.VIT_BF16, nmb, 0 if first == "last_cls_bwd=0" else 2, params,
                 last_cls=0 if first == "last_cls=0" else 1)
    _fwd_bwd(m, px1, lab1)
    m.set_option("last_cls", 1)
    m.set_option("last_cls_bwd", 2)
    la, za, ga = _fwd_bwd(m, px2, lab2)
    m.close()
    m = _trainer(v, cfg, B, v.VIT_BF16, nmb, 2, params)
    lb, zb, gb = _fwd_bwd(m, px2, lab2)
    m.close()
    assert np.float32(la).tobytes() == np.float32(lb).tobytes(), (la, lb)
    _same_bits(za, zb, "logits")
    _same_bits(ga, gb, "grads")


def _hits(v, cfg, B, nmb, bwd):
    params, px, lab = _inputs(v, cfg, B)
    m = _trainer(v, cfg, B, v.VIT_BF16, nmb, bwd, params)
    m.set_batch(px, lab)
    m.sync()
    v.kernel_hits_reset()
    m.zero_grad()
    m.forward()
    m.backward()
    m.grads()
    hits = v.kernel_hits()
    m.close()
    return hits


def test_launch_counters(gpu):
    """B = 64, two micro-batch streams: the whole kernel_hits vector equals the last_cls_bwd=0 step's,
    and the weight gradients did run on the 256x128 engine."""
    v = gpu
    cfg = _cfg(v)
    off = _hits(v, cfg, 64, 2, 0)
    assert off[v.HIT_GEMM_256x128 + 7] >= 4 * cfg.num_layers
    for bwd in (1, 2):
        hits = _hits(v, cfg, 64, 2, bwd)
        assert np.array_equal(hits, off), (bwd, np.nonzero(hits != off))


@pytest.mark.parametrize("prec_name", ["VIT_FP8", "VIT_FP32"])
def test_option_ignored_outside_bf16(gpu, prec_name):
    """fp8 and fp32 mode, test_h64 at B = 4: the option changes nothing."""
    v = gpu
    prec = getattr(v, prec_name)
    cfg = v.data.CONFIGS["test_h64"]
    params, px, lab = _inputs(v, cfg, 4)
    outs = []
    for bwd in (0, 1, 2):
        m = _trainer(v, cfg, 4, prec, 2, bwd, params)
        outs.append(_fwd_bwd(m, px, lab))
        m.close()
    for k in (1, 2):
        assert np.float32(outs[k][0]).tobytes() == np.float32(outs[0][0]).tobytes()
        _same_bits(outs[k][1], outs[0][1], "logits")
        _same_bits(outs[k][2], outs[0][2], "grads")
