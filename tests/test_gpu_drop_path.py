"""Stochastic depth on the GPU: the row-scaled residual epilogue (epi 12) at op level on
every engine that serves it, and vit_trainer_set_drop_path in fp32 and bf16 mode.

Op level, per shape: row scale 1 gives the bits of epi 5, 0 gives C == aux, 2 gives the bits of epi 5
run with 2 B and 2 bias (power-of-two scaling is exact), and a mixed per-row table gives the bits of
numpy's aux + float32(rs * y) with y the epi 0 output of the same call.

Trainer: the production-test geometry of tests/test_gpu_last_cls.py (C = 256, 4 heads, 2 layers,
224^2 / 16), the smallest that reaches the 256x256 engines with two micro-batches; B = 8, and B = 4 for
the runs against the CPU reference (tests/droppath_ref.py).  The exact identities (scale 2 = doubled
projection, scale 0 = zeroed projection, all ones = no table) need no tolerance.
"""
import numpy as np
import pytest

import droppath_ref
import parity

pytestmark = pytest.mark.gpu

EPI_F32_STORE, EPI_F32_RESID, EPI_F32_RESID_RS = 0, 5, 12
VALUES = np.array([0.0, 1.0, 4.0 / 3.0, 2.0], np.float32)  # dropped, kept, kept at p = 0.25 and at p = 0.5


def D(v, a, dt):
    return v.DeviceArray.from_numpy(np.ascontiguousarray(a), dt)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------ op level
def _gemm(v, op, epi, M, N, K, ld, gathered, rs=None, ld_rs=1, scale_b=1.0):
    """C (epilogue)= A . W^T on the rows m * ld / N of the dense [rows, N] tensors; returns C (dense)."""
    Wd = op["W"] if scale_b == 1.0 else op["W2"]
    bias = op["bias"] if scale_b == 1.0 else op["bias2"]
    C = D(v, op["c0"], np.float32)
    lda = ld // N * K
    if epi == EPI_F32_RESID_RS:
        v.call("gemm_bf16_fused_rowscale", C, None, ld, op["aux"], ld, op["A"], lda, 1, Wd, K, 1, bias, None, M, N, K,
               epi, gathered, 0, rs, ld_rs)
    else:
        v.call("gemm_bf16_fused_rows", C, None, ld, op["aux"] if epi == EPI_F32_RESID else None, ld, op["A"], lda, 1,
               Wd, K, 1, bias, None, M, N, K, epi, gathered, 0)
    return C.numpy()


def _operands(v, rows, N, K, seed):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(rows, K)).astype(np.float32)
    w = (rng.normal(size=(N, K)) / np.sqrt(K)).astype(np.float32)
    bias = rng.normal(size=N).astype(np.float32)
    aux = rng.normal(size=(rows, N)).astype(np.float32)
    c0 = np.full((rows, N), 777.0, np.float32)  # rows a gathered call leaves alone keep this
    wb = v.bf16_bits(w).reshape(N, K)
    w2 = v.bf16_bits(2.0 * v.bf16_to_f32(wb)).reshape(N, K)  # exact: a power of two
    return dict(A=D(v, v.bf16_bits(a).reshape(rows, K), np.uint16), W=D(v, wb, np.uint16), W2=D(v, w2, np.uint16),
                bias=D(v, bias, np.float32), bias2=D(v, 2.0 * bias, np.float32), aux=D(v, aux, np.float32),
                aux_np=aux, c0=c0)


def _check_shape(v, M, N, K, stride, hit_base):
    """stride 1: a dense call; > 1: a row-gathered call on rows m * stride."""
    gathered = int(stride > 1)
    rows = M * stride
    ld = stride * N
    op = _operands(v, rows, N, K, seed=M * 7 + N + K)
    sel = np.arange(M) * stride
    rng = np.random.default_rng(M + K)
    table = {"ones": np.ones(rows, np.float32), "zeros": np.zeros(rows, np.float32),
             "twos": np.full(rows, 2.0, np.float32),
             "mixed": rng.choice(VALUES, size=rows)}
    table["mixed"][sel[:4]] = VALUES  # all four occur
    e5 = _gemm(v, op, EPI_F32_RESID, M, N, K, ld, gathered)
    e5x2 = _gemm(v, op, EPI_F32_RESID, M, N, K, ld, gathered, scale_b=2.0)
    y = _gemm(v, op, EPI_F32_STORE, M, N, K, ld, gathered)
    v.kernel_hits_reset()
    out = {k: _gemm(v, op, EPI_F32_RESID_RS, M, N, K, ld, gathered, D(v, t, np.float32), stride)
           for k, t in table.items()}
    hits = v.kernel_hits()
    assert hits[hit_base + EPI_F32_RESID_RS] == len(table), hits[:48]
    assert np.array_equal(_bits(out["ones"][sel]), _bits(e5[sel]))
    assert np.array_equal(_bits(out["zeros"][sel]), _bits(op["aux_np"][sel]))
    assert np.array_equal(_bits(out["twos"][sel]), _bits(e5x2[sel]))
    rs = table["mixed"][sel]
    want = op["aux_np"][sel] + (rs[:, None] * y[sel]).astype(np.float32)
    assert np.array_equal(_bits(out["mixed"][sel]), _bits(want))
    dropped = rs == 0.0
    assert dropped.any() and np.array_equal(_bits(out["mixed"][sel][dropped]), _bits(op["aux_np"][sel][dropped]))
    if gathered:  # the rows between the gathered ones are never written
        rest = np.setdiff1d(np.arange(rows), sel)
        for k in out:
            assert np.all(out[k][rest] == 777.0), k


@pytest.mark.parametrize("M,N,K", [(260, 256, 256), (788, 256, 1024)])
def test_rowscale_epilogue_256_engine(gpu, M, N, K):
    _check_shape(gpu, M, N, K, 1, gpu.HIT_GEMM_256x256)


def test_rowscale_epilogue_256_one_tile_form(gpu):
    """variant 2: the one-tile-per-workgroup 256x256 form (the wave-tile staged epilogue)."""
    v = gpu
    v.lib().gemm_bf16_set_variant(2)
    try:
        _check_shape(v, 260, 256, 256, 1, v.HIT_GEMM_256x256)
    finally:
        v.lib().gemm_bf16_set_variant(0)


def test_rowscale_epilogue_variant_11_declines(gpu):
    """variant 11: the ping-pong engine does not take epi 12; the call runs on the default engine, same bits."""
    v = gpu
    M, N, K = 260, 256, 256
    op = _operands(v, M, N, K, seed=11)
    rs = D(v, np.resize(VALUES, M), np.float32)
    want = _gemm(v, op, EPI_F32_RESID_RS, M, N, K, N, 0, rs, 1)
    v.lib().gemm_bf16_set_variant(11)
    try:
        v.kernel_hits_reset()
        got = _gemm(v, op, EPI_F32_RESID_RS, M, N, K, N, 0, rs, 1)
        hits = v.kernel_hits()
    finally:
        v.lib().gemm_bf16_set_variant(0)
    assert hits[v.HIT_GEMM_PP] == 0 and hits[v.HIT_GEMM_256x256 + EPI_F32_RESID_RS] == 1
    assert np.array_equal(_bits(got), _bits(want))


def test_rowscale_epilogue_128_engine(gpu):
    _check_shape(gpu, 96, 128, 128, 1, gpu.HIT_GEMM_128)


def test_rowscale_epilogue_row_gathered(gpu):
    """M = 4 rows at stride 197 of the dense tensors (the last block's CLS rows), ld_row_scale = 197."""
    _check_shape(gpu, 4, 256, 256, 197, gpu.HIT_GEMM_256x256)


def test_rowscale_rejects_bad_arguments(gpu):
    v = gpu
    op = _operands(v, 96, 128, 128, seed=1)
    C = D(v, op["c0"], np.float32)
    with pytest.raises(v.VitError):  # no row scales
        v.call("gemm_bf16_fused_rowscale", C, None, 128, op["aux"], 128, op["A"], 128, 1, op["W"], 128, 1, op["bias"],
               None, 96, 128, 128, EPI_F32_RESID_RS, 0, 0, None, 1)
    with pytest.raises(v.VitError):  # another epilogue
        v.call("gemm_bf16_fused_rowscale", C, None, 128, op["aux"], 128, op["A"], 128, 1, op["W"], 128, 1, op["bias"],
               None, 96, 128, 128, EPI_F32_RESID, 0, 0, op["bias"], 1)


# ------------------------------------------------------------------ trainer


def _cfg(v):
    return v.data.VitCfg("prod_l2", img=224, patch=16, channels=256, num_layers=2, num_heads=4, num_classes=1000)


def _mixed_table(L, B, shift=0):
    """every value of VALUES in every (layer, branch) row when B >= 4, a different image order per row"""
    t = np.empty((L, 2, B), np.float32)
    for l in range(L):
        for br in range(2):
            t[l, br] = VALUES[(np.arange(B) + 2 * l + br + shift) % 4]
    return t


_inputs_cache = {}


def _inputs(v, cfg, B, seed=5):
    key = (cfg.name, B, seed)
    if key not in _inputs_cache:
        params = v.data.init_params(cfg, "parity", seed=3)
        px, lab = v.data.synthetic_batch(cfg, B, seed=seed)
        _inputs_cache[key] = (params, px, lab)
    return _inputs_cache[key]


def _fwd_bwd(m, px, lab, table=None):
    m.set_batch(px, lab)
    m.zero_grad()
    if table is not None:
        m.set_drop_path(table)
    loss = m.forward()
    m.backward()
    return loss, m.logits().copy(), m.grads()


def _step(v, cfg, B, params, px, lab, table=None, prec=None, options=(), concurrency=True):
    m = v.ViT.build(cfg, B, v.VIT_BF16 if prec is None else prec, params=params)
    m.set_concurrency(concurrency)
    for k, val in options:
        m.set_option(k, val)
    out = _fwd_bwd(m, px, lab, table)
    m.close()
    return out


def _same_step(a, b, cfg, what=""):
    (l1, z1, g1), (l0, z0, g0) = a, b
    assert np.float32(l1).tobytes() == np.float32(l0).tobytes(), (what, l1, l0)
    assert np.array_equal(_bits(z1), _bits(z0)), (what, "logits")
    t1, t0 = cfg.split(g1), cfg.split(g0)
    for name in t1:
        assert np.array_equal(_bits(t1[name]), _bits(t0[name])), (what, name)


def _layer(cfg, flat, name, l):
    """view of layer l of tensor `name` in a canonical flat array"""
    t = cfg.split(flat)[name]
    n = t.size // cfg.num_layers
    return t.reshape(-1)[l * n:(l + 1) * n]


PROJ = {0: ("attprojw", "attprojb"), 1: ("fcprojw", "fcprojb")}


def _scaled_params(cfg, params, l, br, factor):
    p = np.array(params, np.float32, copy=True)
    for name in PROJ[br]:
        _layer(cfg, p, name, l)[:] *= np.float32(factor)
    return p


def _gate(cfg, got, ref, rule, label):
    loss, z, g = got
    loss_r, z_r, g_r = ref
    lrel = abs(loss - loss_r) / abs(loss_r)
    bad, rep = parity.check(parity.tensors(cfg, z, g, z_r, g_r), rule)
    print(f"\n{label}: loss {lrel:.2e}, {parity.summary(rep)}")
    assert lrel <= rule["loss"], (label, lrel)
    assert not bad, (label, bad)


def test_fp32_mixed_table_vs_reference(gpu, oracle32):
    v = gpu
    import os
    from conftest import ROOT
    zf = np.load(os.path.join(ROOT, "tests", "golden", "test.npz"))
    cfg, params, px, lab = v.data.CONFIGS["test"], zf["params"], zf["pixels"], zf["labels"]
    B = px.shape[0]
    table = np.array([[[0.0, 1.0], [4.0 / 3.0, 2.0]], [[2.0, 4.0 / 3.0], [1.0, 0.0]]], np.float32)
    assert table.shape == (cfg.num_layers, 2, B)
    ref = droppath_ref.step(oracle32, cfg, params, px, lab, table)
    got = _step(v, cfg, B, params, px, lab, table, prec=v.VIT_FP32)
    _gate(cfg, got, ref, parity.FP32, "fp32 drop path")
    free = _step(v, cfg, B, params, px, lab, None, prec=v.VIT_FP32)
    ones = _step(v, cfg, B, params, px, lab, np.ones_like(table), prec=v.VIT_FP32)
    _same_step(ones, free, cfg, "fp32 all ones")
    assert not np.array_equal(got[1], free[1])


@pytest.fixture(scope="module")
def ref_b4(gpu, oracle32):
    v = gpu
    cfg = _cfg(v)
    params, px, lab = _inputs(v, cfg, 4)
    table = _mixed_table(cfg.num_layers, 4)
    return dict(cfg=cfg, params=params, px=px, lab=lab, table=table,
                ref=droppath_ref.step(oracle32, cfg, params, px, lab, table))


@pytest.mark.parametrize("concurrency", [True, False])
def test_bf16_mixed_table_vs_reference(gpu, ref_b4, concurrency):
    v, r = gpu, ref_b4
    got = _step(v, r["cfg"], 4, r["params"], r["px"], r["lab"], r["table"], concurrency=concurrency)
    _gate(r["cfg"], got, r["ref"], parity.BF16, f"bf16 drop path, concurrency {concurrency}")


def test_bf16_all_ones_is_no_table_bitwise(gpu):
    v = gpu
    cfg, B = _cfg(v), 8
    params, px, lab = _inputs(v, cfg, B)
    m = v.ViT.build(cfg, B, v.VIT_BF16, params=params)
    bytes0 = m.device_bytes()
    v.kernel_hits_reset()
    free = _fwd_bwd(m, px, lab)
    m.sync()
    h_free = v.kernel_hits()
    assert m.drop_path() is None and m.device_bytes() == bytes0  # nothing allocated until a table is set
    m.close()
    # a step that never set a table launches no row-scaled epilogue
    for base in (v.HIT_GEMM_128, v.HIT_GEMM_256x256, v.HIT_GEMM_256x128):
        assert h_free[base + EPI_F32_RESID_RS] == 0
    m = v.ViT.build(cfg, B, v.VIT_BF16, params=params)
    v.kernel_hits_reset()
    ones = _fwd_bwd(m, px, lab, np.ones((cfg.num_layers, 2, B), np.float32))
    m.sync()
    h_ones = v.kernel_hits()
    assert m.device_bytes() > bytes0
    m.close()
    _same_step(ones, free, cfg, "all ones")
    # ... and the table moves exactly the residual-epilogue GEMMs from epi 5 to epi 12, nothing else counted
    moved = h_free.copy()
    for base in (v.HIT_GEMM_128, v.HIT_GEMM_256x256):
        moved[base + EPI_F32_RESID_RS] = moved[base + EPI_F32_RESID]
        moved[base + EPI_F32_RESID] = 0
    assert np.array_equal(h_ones, moved), np.nonzero(h_ones != moved)
    assert h_ones[v.HIT_GEMM_256x256 + EPI_F32_RESID_RS] == 2 * 2 * cfg.num_layers  # 2 branches x 2 micro-batches


@pytest.mark.parametrize("l,br", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_bf16_scale_two_is_doubled_projection(gpu, l, br):
    v = gpu
    cfg, B = _cfg(v), 8
    params, px, lab = _inputs(v, cfg, B)
    table = np.ones((cfg.num_layers, 2, B), np.float32)
    table[l, br] = 2.0
    got = _step(v, cfg, B, params, px, lab, table)
    dbl = _step(v, cfg, B, _scaled_params(cfg, params, l, br, 2.0), px, lab)
    assert np.float32(got[0]).tobytes() == np.float32(dbl[0]).tobytes()
    assert np.array_equal(_bits(got[1]), _bits(dbl[1]))
    tg, td = cfg.split(got[2]), cfg.split(dbl[2])
    for name in tg:
        a, b = np.array(tg[name], copy=True), np.array(td[name], copy=True)
        if name in PROJ[br]:  # the scaled branch's own tensors: exactly twice the doubled run's, in layer l
            _layer_view = lambda x: x.reshape(cfg.num_layers, -1)[l]  # noqa: E731
            _layer_view(b)[:] = np.float32(2.0) * _layer_view(b)
            assert np.abs(_layer_view(a)).max() > 0
        assert np.array_equal(_bits(a), _bits(b)), name


@pytest.mark.parametrize("l,br", [(0, 1), (1, 0), (1, 1)])
def test_bf16_one_image_dropped_is_zeroed_projection(gpu, l, br):
    v = gpu
    cfg, B, b0 = _cfg(v), 8, 5
    params, px, lab = _inputs(v, cfg, B)
    table = np.ones((cfg.num_layers, 2, B), np.float32)
    table[l, br, b0] = 0.0
    got = _step(v, cfg, B, params, px, lab, table)
    zeroed = _step(v, cfg, B, _scaled_params(cfg, params, l, br, 0.0), px, lab)
    free = _step(v, cfg, B, params, px, lab)
    assert np.all(got[1][b0] == zeroed[1][b0])
    rest = np.arange(B) != b0
    assert np.array_equal(_bits(got[1][rest]), _bits(free[1][rest]))  # the other images are untouched
    assert not np.array_equal(got[1][b0], free[1][b0])


@pytest.mark.parametrize("l", [0, 1])
def test_bf16_all_images_dropped_in_mlp(gpu, l):
    v = gpu
    cfg, B = _cfg(v), 8
    params, px, lab = _inputs(v, cfg, B)
    table = np.ones((cfg.num_layers, 2, B), np.float32)
    table[l, 1] = 0.0
    got = _step(v, cfg, B, params, px, lab, table)
    zeroed = _step(v, cfg, B, _scaled_params(cfg, params, l, 1, 0.0), px, lab)
    for name in ("fcw", "fcb", "ln2w", "ln2b"):
        assert np.all(_layer(cfg, got[2], name, l) == 0.0), name
    assert np.all(got[1] == zeroed[1]) and got[0] == zeroed[0]
    tg, tz = cfg.split(got[2]), cfg.split(zeroed[2])
    for name in tg:
        if name in PROJ[1]:  # (the dropped projection's own gradient is zero in layer l; the zeroed run's is not)
            a, b = tg[name].reshape(cfg.num_layers, -1), tz[name].reshape(cfg.num_layers, -1)
            assert np.all(a[l] == 0.0)
            assert np.all(np.delete(a, l, 0) == np.delete(b, l, 0)), name
        else:
            assert np.all(tg[name] == tz[name]), name


def test_bf16_last_cls_settings_bitwise(gpu):
    v = gpu
    cfg, B = _cfg(v), 8
    params, px, lab = _inputs(v, cfg, B)
    table = _mixed_table(cfg.num_layers, B, shift=1)
    base = _step(v, cfg, B, params, px, lab, table, options=(("last_cls", 0),))
    assert np.isfinite(base[0]) and np.isfinite(base[2]).all()
    for bwd in (0, 1, 2):
        got = _step(v, cfg, B, params, px, lab, table, options=(("last_cls", 1), ("last_cls_bwd", bwd)))
        _same_step(got, base, cfg, f"last_cls 1, last_cls_bwd {bwd}")
    free = _step(v, cfg, B, params, px, lab)
    assert not np.array_equal(base[1], free[1])


# ------------------------------------------------------------------ lifecycle
def test_lifecycle(gpu):
    v = gpu
    cfg, B = _cfg(v), 8
    params, px, lab = _inputs(v, cfg, B)
    table = _mixed_table(cfg.num_layers, B)
    free = _step(v, cfg, B, params, px, lab)
    m = v.ViT.build(cfg, B, v.VIT_BF16, params=params)
    assert m.drop_path() is None
    masked = _fwd_bwd(m, px, lab, table)
    assert np.array_equal(m.drop_path(), table)
    assert not np.array_equal(masked[1], free[1])
    # one-shot: the next step runs without a table
    again = _fwd_bwd(m, px, lab)
    _same_step(again, free, cfg, "the step after a masked one")
    assert m.drop_path() is None
    # evaluate() and a forward without labels never drop and leave the table pending
    m.set_drop_path(table)
    m.evaluate(px, lab)
    assert np.array_equal(_bits(m.logits()), _bits(free[1]))
    m.forward(px, None)
    assert np.array_equal(_bits(m.logits()), _bits(free[1]))
    m.set_batch(px, lab)
    m.zero_grad()
    m.forward()
    assert np.array_equal(_bits(m.logits()), _bits(masked[1])) and np.array_equal(m.drop_path(), table)
    m.backward()
    assert np.array_equal(_bits(m.grads()), _bits(masked[2]))
    # a bad entry is rejected and the pending table stays
    other = _mixed_table(cfg.num_layers, B, shift=2)
    m.set_drop_path(other)
    for bad in (np.nan, -1.0, np.inf, -np.inf):
        t = other.copy()
        t[1, 0, 3] = bad
        with pytest.raises(v.VitError):
            m.set_drop_path(t)
    m.set_batch(px, lab)
    m.forward()
    assert np.array_equal(m.drop_path(), other)
    # None clears a pending table
    m.set_drop_path(table)
    m.set_drop_path(None)
    m.forward()
    assert m.drop_path() is None and np.array_equal(_bits(m.logits()), _bits(free[1]))
    # train_step consumes a table too
    m.set_drop_path(table)
    m.train_step(0.0)
    m.sync()
    assert np.array_equal(m.drop_path(), table) and np.array_equal(_bits(m.logits()), _bits(masked[1]))
    m.close()


def test_fp8_trainer_rejects(gpu):
    v = gpu
    cfg = v.data.CONFIGS["test_h64"]
    m = v.ViT.build(cfg, 2, v.VIT_FP8, params=v.data.init_params(cfg, "parity", seed=3))
    with pytest.raises(v.VitError, match="not supported in fp8 mode"):
        m.set_drop_path(np.ones((cfg.num_layers, 2, 2), np.float32))
    m.close()
