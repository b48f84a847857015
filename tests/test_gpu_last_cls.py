"""Option last_cls: in bf16 mode the last block's attention projection, LayerNorm 2,
fc + GELU and fcproj and the fc / attention-projection input gradients run on the B CLS rows only (the
head reads nothing else), in place at row stride T, on the engines of the full-size step.

Shapes: the production-test geometry (C=256, 4 heads, 2 layers, 224^2 / 16: N >= 256 and K % 64 == 0,
so the trimmed GEMMs are one ragged 256x256 row panel of M = 2, 3, 4 or 8 rows; at B = 2 on two
streams the full-size GEMMs have 197 rows and run, like the trimmed ones of 1 row, on the 128x128
kernel) and test_h64 at B = 4 (C = 128: below the 256x256 engine's shapes), each with one and two
micro-batch streams.

The CLS rows come from the same tile code in the same K order and every skipped row was an exact zero
or is never read; the kernels that take the last block's small gradients' partial sums (fc_b in the
fcproj dgrad, ln2_w / ln2_b / attproj_b in LayerNorm 2 backward) stay full size, so those sums keep
their grouping: loss, logits and every gradient are bit-identical to last_cls=0 (which also meets the
project's fp32 rule, tests/parity.py FP32, for the four tensors the trimming could have regrouped).
"""
import numpy as np
import pytest

import parity

pytestmark = pytest.mark.gpu

def _cfg(v):
    return v.data.VitCfg("prod_l2", img=224, patch=16, channels=256, num_layers=2, num_heads=4, num_classes=1000)


_inputs_cache = {}


def _inputs(v, cfg, B, seed=5):
    key = (cfg.name, B, seed)
    if key not in _inputs_cache:
        params = v.data.init_params(cfg, "parity", seed=3)
        px, lab = v.data.synthetic_batch(cfg, B, seed=seed)
        _inputs_cache[key] = (params, px, lab)
    return _inputs_cache[key]


def _trainer(v, cfg, B, prec, nmb, last_cls, params):
    m = v.ViT.build(cfg, B, prec, params=params)
    m.set_concurrency(True)
    m.set_option("microbatch", nmb)
    m.set_option("last_cls", last_cls)
    return m


def _fwd_bwd(m, px, lab):
    m.set_batch(px, lab)
    m.zero_grad()
    loss = m.forward()
    m.backward()
    return loss, m.logits().copy(), m.grads()


def _step(v, cfg, B, prec, nmb, last_cls, params, px, lab):
    m = _trainer(v, cfg, B, prec, nmb, last_cls, params)
    out = _fwd_bwd(m, px, lab)
    m.close()
    return out


def _same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), \
        (what, int(np.sum(a.view(np.uint32) != b.view(np.uint32))))


@pytest.mark.parametrize("B,nmb", [(2, 1), (2, 2), (3, 1), (3, 2), (8, 1), (8, 2)])
def test_on_equals_off(gpu, B, nmb):
    """One zero_grad / forward / backward, last_cls on against off, same seeded inputs."""
    v = gpu
    cfg = _cfg(v)
    params, px, lab = _inputs(v, cfg, B)
    l1, z1, g1 = _step(v, cfg, B, v.VIT_BF16, nmb, 1, params, px, lab)
    l0, z0, g0 = _step(v, cfg, B, v.VIT_BF16, nmb, 0, params, px, lab)
    assert np.isfinite(l1) and np.isfinite(g1).all()
    assert np.float32(l1).tobytes() == np.float32(l0).tobytes(), (l1, l0)
    _same_bits(z1, z0, "logits")
    t1, t0 = cfg.split(g1), cfg.split(g0)
    for name in t1:
        _same_bits(t1[name], t0[name], name)


@pytest.fixture(scope="module")
def h64_ref(gpu, oracle32):
    import oracle_ctypes as oc
    from test_gpu_model import oracle_step
    v = gpu
    cfg = v.data.CONFIGS["test_h64"]
    params, px, lab = _inputs(v, cfg, 4)
    loss, logits, g = oracle_step(oc, oracle32, cfg, params, px, lab)
    return dict(cfg=cfg, params=params, px=px, lab=lab, loss=loss, logits=logits, grads=g)


@pytest.mark.parametrize("nmb", [1, 2])
def test_small_model_on_and_off_vs_oracle(gpu, h64_ref, nmb):
    """test_h64, B = 4: both settings against the fp32 CPU oracle, and their logits against each other."""
    v = gpu
    r = h64_ref
    outs = {}
    for on in (1, 0):
        loss, z, g = _step(v, r["cfg"], 4, v.VIT_BF16, nmb, on, r["params"], r["px"], r["lab"])
        lrel = abs(loss - r["loss"]) / abs(r["loss"])
        bad, rep = parity.check(parity.tensors(r["cfg"], z, g, r["logits"], r["grads"]), parity.BF16)
        print(f"\ntest_h64 nmb={nmb} last_cls={on}: loss {lrel:.2e}, {parity.summary(rep)}")
        assert lrel <= parity.BF16["loss"], (on, lrel)
        assert not bad, (on, bad)
        outs[on] = z
    bad, rep = parity.check({"logits": (outs[1], outs[0])}, parity.BF16)
    assert not bad, bad


@pytest.mark.parametrize("nmb", [1, 2])
@pytest.mark.parametrize("first", [0, 1])
def test_no_stale_rows_leak(gpu, nmb, first):
    """A step on batch 1 (last_cls off: every buffer then holds real non-CLS rows; or on: the shared
    gradient scratch ends the step holding layer 0's rows), then last_cls on and a step on batch 2:
    the same bits as a fresh trainer that had it on from the start and saw only batch 2."""
    v = gpu
    cfg = _cfg(v)
    B = 8
    params, px1, lab1 = _inputs(v, cfg, B, seed=5)
    _, px2, lab2 = _inputs(v, cfg, B, seed=11)
    m = _trainer(v, cfg, B, v.VIT_BF16, nmb, first, params)
    _fwd_bwd(m, px1, lab1)
    m.set_option("last_cls", 1)
    la, za, ga = _fwd_bwd(m, px2, lab2)
    m.close()
    lb, zb, gb = _step(v, cfg, B, v.VIT_BF16, nmb, 1, params, px2, lab2)
    assert np.float32(la).tobytes() == np.float32(lb).tobytes(), (la, lb)
    _same_bits(za, zb, "logits")
    _same_bits(ga, gb, "grads")


@pytest.mark.parametrize("nmb", [1, 2])
def test_train_steps_repeatable(gpu, nmb):
    """Three consecutive train_steps with last_cls on, on two trainers, and with it off on a third:
    bit-identical logits and parameters (the per-step clears are ordered against the previous step's
    readers and this step's writers by events; a clear that raced either would change some bits on
    some run; and since every gradient keeps its bits, so does the whole trajectory)."""
    v = gpu
    cfg = _cfg(v)
    B = 8
    params, px, lab = _inputs(v, cfg, B)
    runs = []
    for on in (1, 1, 0):
        m = _trainer(v, cfg, B, v.VIT_BF16, nmb, on, params)
        m.set_batch(px, lab)
        for _ in range(3):
            m.train_step(0.05)
        m.sync()
        z = m.logits().copy()
        p = m.params()
        m.close()
        assert np.isfinite(p).all()
        runs.append((z, p))
    for k in (1, 2):
        _same_bits(runs[0][0], runs[k][0], f"logits (run {k})")
        _same_bits(runs[0][1], runs[k][1], f"params (run {k})")


def _hits(v, cfg, B, nmb, last_cls):
    params, px, lab = _inputs(v, cfg, B)
    m = _trainer(v, cfg, B, v.VIT_BF16, nmb, last_cls, params)
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


@pytest.mark.parametrize("B", [8, 64])
def test_launch_mix(gpu, B):
    """Two micro-batch streams: the trimmed launches stay on the 256x256 engine with their epilogues, so
    every launch counter equals the last_cls=0 step's and the per-layer mix is the production step's
    (tests/test_gpu_production.py).  B = 8: trimmed panels of 4 rows.  Its weight gradients reduce over
    K = 8 x 197 = 1576 tokens, not a multiple of the 256x128 engine's 64, so with the option on or off
    they are the one class on the 128x128 split-K kernel (counter 7) and never reach the 256x128
    counter; B = 64 (64 x 197 = 197 x 64, the shard shape of the production DP test) is the smallest
    batch at which the production test's whole set of equalities applies."""
    v = gpu
    cfg = _cfg(v)
    nmb, L = 2, cfg.num_layers
    hits = _hits(v, cfg, B, nmb, 1)
    off = _hits(v, cfg, B, nmb, 0)
    assert np.array_equal(hits, off), np.nonzero(hits != off)
    G1, G2, G4 = v.HIT_GEMM_128, v.HIT_GEMM_256x256, v.HIT_GEMM_256x128
    fallback = hits[G1:G1 + 16].copy()
    if (B * 197) % 64:
        assert fallback[7] == off[G1 + 7] == 4 * L  # the weight gradients' slabs
        fallback[7] = 0
    else:
        assert hits[G4 + 7] >= 4 * L
    assert fallback.sum() == 0, "128x128 fallback ran"
    assert hits[G2 + 3] >= 4 * L * nmb
    assert hits[G2 + 5] == 2 * L * nmb
    assert hits[G2 + 8] == L * nmb
    assert hits[G2 + 9] == L * nmb
    assert hits[v.HIT_SPLITK_REDUCE] == hits[G4 + 7] + hits[G2 + 7] + hits[G1 + 7] + hits[v.HIT_GEMM_F32 + 7]
    assert hits[v.HIT_ATTN_FWD_MFMA] == L * nmb and hits[v.HIT_ATTN_BWD_PERSISTENT] == L * nmb


@pytest.mark.parametrize("prec_name", ["VIT_FP8", "VIT_FP32"])
def test_option_ignored_outside_bf16(gpu, prec_name):
    """last_cls=1 in fp8 and fp32 mode leaves the step bit-identical to last_cls=0."""
    v = gpu
    prec = getattr(v, prec_name)
    cfg = v.data.CONFIGS["test_h64"]
    params, px, lab = _inputs(v, cfg, 4)
    l1, z1, g1 = _step(v, cfg, 4, prec, 2, 1, params, px, lab)
    l0, z0, g0 = _step(v, cfg, 4, prec, 2, 0, params, px, lab)
    assert np.float32(l1).tobytes() == np.float32(l0).tobytes(), (l1, l0)
    _same_bits(z1, z0, "logits")
    _same_bits(g1, g0, "grads")
