"""Momentum SGD on the GPU (include/vit_trainer.h vit_trainer_set_sgd): the sgd_momentum_step op
and the momentum instantiations of the optimizer kernels against vit.sgd.sgd_ref (numpy fp32, every operation
rounded on its own) fed with the device's own gradients and previous parameters.  Every comparison is bit-exact.

Shapes: CONFIGS["test"] with B = 3 in fp32 mode, CONFIGS["test_h64"] with B = 4 in bf16 / fp8 mode (the
fixtures of tests/test_gpu_ema.py): tensors shorter than a tile, short last tiles and the arena's padding."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = float("inf")
LR = 0.01
ALR = 3e-3
HP = dict(beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.05)
D = 0.9
PRECS = {"fp32": ("VIT_FP32", "test", 3), "bf16": ("VIT_BF16", "test_h64", 4), "fp8": ("VIT_FP8", "test_h64", 4)}
MULS = np.array([0.0, 0.25, 0.65, 0.65 ** 2, 1.0, 1.5], F32)
# (momentum, dampening, weight decay, nesterov)
PLAIN = (0.9, 0.0, 0.0, False)
NESTEROV = (0.9, 0.0, 5e-4, True)
DAMPENED = (0.9, 0.1, 5e-4, False)
SETTINGS = {"plain": PLAIN, "nesterov_wd": NESTEROV, "dampening_wd": DAMPENED}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def setup(v, prec, seed=3):
    prec_name, name, B = PRECS[prec]
    cfg = v.data.CONFIGS[name]
    params = v.data.init_params(cfg, "parity", seed=seed)
    px, lab = v.data.synthetic_batch(cfg, B, seed=seed + 2)
    return cfg, B, getattr(v, prec_name), params, px, lab


def build(v, prec, nmb=None, seed=3, params=None):
    cfg, B, p, params0, px, lab = setup(v, prec, seed)
    m = v.ViT.build(cfg, B, p, params=params0 if params is None else params)
    m.set_concurrency(True)
    if nmb is not None:
        m.set_option("microbatch", nmb)
    m.set_batch(px, lab)
    return m


def draw(cfg, seed):
    rng = np.random.default_rng(seed)
    shape = (20, cfg.num_layers)
    return rng.choice(MULS, size=shape).astype(F32), rng.choice(MULS, size=shape).astype(F32)


def slices(v, cfg):
    """(ti, l, slice of the canonical flat arrays) of every (tensor, layer)"""
    L, off = cfg.num_layers, 0
    for ti, (name, size) in enumerate(zip(v.data.PARAM_NAMES, cfg.param_sizes())):
        if name in v.data.LAYER_PARAMS:
            n = size // L
            for l in range(L):
                yield ti, l, slice(off + l * n, off + (l + 1) * n)
        else:
            yield ti, 0, slice(off, off + size)
        off += size


def expect(v, cfg, p, g, b, first, lr, s, muls=None, c=None):
    """sgd_ref over the whole model: one call without groups, per (tensor, layer) with lr_e = fl(lr * lr_mul)
    and wd_e = fl(wd * wd_mul) under groups.  Returns (p', b')."""
    mu, damp, wd, nesterov = s
    if muls is None:
        return v.sgd.sgd_ref(p, g, b, first, lr, mu, damp, wd, nesterov, c=c)
    lr_mul, wd_mul = muls
    po, bo = np.empty_like(p), np.empty_like(p)
    for ti, l, sl in slices(v, cfg):
        lr_e = F32(F32(lr) * lr_mul[ti, l])
        wd_e = F32(F32(wd) * wd_mul[ti, l])
        po[sl], bo[sl] = v.sgd.sgd_ref(p[sl], g[sl], None if b is None else b[sl], first, lr_e, mu, damp, wd_e,
                                       nesterov, c=c)
    return po, bo


def clip_coef(max_norm, n):
    c = F32(max_norm) / (F32(n) + F32(1e-6))
    return c if c < F32(1.0) else F32(1.0)


def arm(m, frac=0.1):
    """a norm-reading step at lr = 0 (the parameters stay), then max_norm = frac * norm: the clip stays active"""
    m.set_grad_clip(INF)
    m.train_step(0.0)
    m.sync()
    n0 = m.grad_norm()
    assert n0 > 0 and np.isfinite(n0)
    m.set_grad_clip(frac * n0)
    return frac * n0


def fwd_bwd(m):
    m.zero_grad()
    m.forward()
    m.backward()


def one_step(m, k=1, lr=LR):
    """step k of a run: through the separate calls first (k = 0), then through the fused train step"""
    if k == 0:
        fwd_bwd(m)
        m.optimizer_step(lr)
    else:
        m.train_step(lr)
    m.sync()


def loss_of(v, m):
    m.forward()
    return float(v.lib().vit_trainer_mean_loss(m.h))


def arena_elems(v, cfg):
    n = ctypes.c_longlong()
    assert v.lib().vit_layout_query(ctypes.byref(v._cfg_c(cfg)), None, None, ctypes.byref(n)) > 0
    return n.value


# ------------------------------------------------------------------ 1. the op
def op_values(n, seed):
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(F32)
    special = np.array([0.0, -0.0, 1e-45, -3e-42, 1.1754942e-38, -1e-38, 1e30, -65504.0], F32)
    k = min(n, special.size)
    a[rng.permutation(n)[:k]] = rng.permutation(special)[:k]
    return a


@pytest.mark.parametrize("n", [0, 1, 3, 5, 4099, 16384 + 5])
def test_sgd_momentum_step_op(gpu, n):
    """pointers one float off a 16-byte boundary; first = 1 then 0; plain and Nesterov, weight decay 0 and 5e-4;
    g holds +0 and -0 (a first step at weight decay 0 copies them into the buffer bit for bit)"""
    v = gpu
    p0, g0, g1 = op_values(n + 2, n), op_values(n + 2, n + 1), op_values(n + 2, n + 2)
    if n >= 2:
        g0[1:3] = [0.0, -0.0]
    junk = op_values(n + 2, n + 3)  # the buffer's content before the first step: not looked at
    v.kernel_hits_reset()
    calls = 0
    for nesterov in (False, True):
        for wd in (0.0, 5e-4):
            pd, bd = v.DeviceArray.from_numpy(p0), v.DeviceArray.from_numpy(junk)
            gd = [v.DeviceArray.from_numpy(g0), v.DeviceArray.from_numpy(g1)]
            want_p, want_b = p0.copy(), junk.copy()
            for k in range(2):
                v.sgd_momentum_step(pd.ptr + 4, gd[k].ptr + 4, bd.ptr + 4, n, 0.05, 0.9, 0.0, wd, nesterov, k == 0)
                calls += n > 0
                g = (g0, g1)[k]
                want_p[1:n + 1], want_b[1:n + 1] = v.sgd.sgd_ref(want_p[1:n + 1], g[1:n + 1], want_b[1:n + 1], k == 0,
                                                                 0.05, 0.9, 0.0, wd, nesterov)
                got_p, got_b = pd.numpy(), bd.numpy()
                bad = np.nonzero((bits(got_p) != bits(want_p)) | (bits(got_b) != bits(want_b)))[0]
                assert bad.size == 0, (nesterov, wd, k, bad[:8])  # (the elements around the range stay)
                if k == 0 and wd == 0.0 and n >= 2:
                    assert same_bits(got_b[1:3], [0.0, -0.0])
            for a in [pd, bd] + gd:
                a.free()
    assert v.kernel_hits()[v.HIT_SGDM] == calls  # n = 0 launches nothing
    # dampening, in the op's scalar form
    if n:
        pd, bd, gd = v.DeviceArray.from_numpy(p0), v.DeviceArray.from_numpy(junk), v.DeviceArray.from_numpy(g1)
        v.sgd_momentum_step(pd, gd, bd, n + 2, 0.05, 0.5, 0.5, 5e-4, False, False)
        want_p, want_b = v.sgd.sgd_ref(p0, g1, junk, False, 0.05, 0.5, 0.5, 5e-4, False)
        assert same_bits(pd.numpy(), want_p) and same_bits(bd.numpy(), want_b)
        for bad in (dict(nesterov=True, momentum=0.0), dict(nesterov=True, dampening=0.1), dict(momentum=-0.1),
                    dict(weight_decay=float("nan")), dict(dampening=INF)):
            with pytest.raises(v.VitError):
                v.sgd_momentum_step(pd, gd, bd, n, 0.05, **bad)
        assert same_bits(pd.numpy(), want_p)
        for a in (pd, bd, gd):
            a.free()


# ------------------------------------------------------------------ 2. the trainer
@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp8"])
def test_trainer_matches_sgd_ref(gpu, prec, setting):
    v = gpu
    cfg = setup(v, prec)[0]
    s = SETTINGS[setting]
    m = build(v, prec)
    m.set_sgd(*s)
    info = m.sgd_info()
    assert (F32(info["momentum"]), F32(info["dampening"]), F32(info["weight_decay"]), info["nesterov"], info["steps"]) \
        == (F32(s[0]), F32(s[1]), F32(s[2]), s[3], 0)
    p, b = m.params(), None
    p_start = p
    v.kernel_hits_reset()
    for k in range(3):
        one_step(m, k)
        p, b = expect(v, cfg, p, m.grads(), b, k == 0, LR, s)
        got_p, got_b = m.params(), m.momentum()
        bad = int((bits(got_p) != bits(p)).sum()), int((bits(got_b) != bits(b)).sum())
        assert bad == (0, 0), (k, bad)
        assert m.sgd_info()["steps"] == k + 1
    assert not same_bits(p, p_start)
    assert v.kernel_hits()[v.HIT_SGDM] >= 3
    # the shadow, the transposed copies and the fp8 copies follow the fp32 values: a fresh trainer built from
    # them computes the same loss bits
    fresh = build(v, prec, params=p)
    assert loss_of(v, m) == loss_of(v, fresh)
    fresh.close()
    m.close()


# ------------------------------------------------------------------ 3. composition
@pytest.mark.parametrize("groups", [False, True], ids=["nogroups", "groups"])
@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp8"])
def test_composition(gpu, prec, clip, groups):
    """clip x parameter groups, the EMA on, fused into the kernels (ema_fused 1) and behind them (0): the eight
    momentum kernels between the two runs.  Both equal sgd_ref + ema_ref and each other."""
    v = gpu
    cfg = setup(v, prec)[0]
    s = NESTEROV
    muls = draw(cfg, 41) if groups else None
    if groups:
        used = [(ti, l) for ti, l, _ in slices(v, cfg)]
        assert any(muls[0][e] == 0 for e in used) and any(muls[0][e] == F32(1.5) for e in used)
        assert any(muls[1][e] == 0 and muls[0][e] != 0 for e in used)  # a segment on the no-decay branch
    runs = []
    for fused in (1, 0):
        m = build(v, prec)
        m.set_option("ema_fused", fused)
        mx = arm(m) if clip else None
        if groups:
            m.set_param_groups(*muls)
        m.set_ema(D)
        m.set_sgd(*s)
        p, b, e = m.params(), None, m.ema()
        out = []
        for k in range(3):
            p_prev, b_prev = p, b
            one_step(m, k)
            c = None
            if clip:
                c = clip_coef(mx, m.grad_norm())
                assert c < 1
            p, b = expect(v, cfg, p, m.grads(), b, k == 0, LR, s, muls, c)
            e = v.ema.ema_ref(e, p, D)
            assert same_bits(m.params(), p) and same_bits(m.momentum(), b) and same_bits(m.ema(), e), (fused, k)
            if groups and k:  # a frozen tensor keeps its bits while its buffer advances
                frozen = [sl for ti, l, sl in slices(v, cfg) if muls[0][ti, l] == 0]
                assert all(same_bits(p[sl], p_prev[sl]) for sl in frozen)
                assert any(not same_bits(b[sl], b_prev[sl]) for sl in frozen)
            out.append((p, b, e, float(v.lib().vit_trainer_mean_loss(m.h))))
        assert m.sgd_info()["steps"] == 3 and m.ema_info()[1] == 3
        if clip:
            assert not same_bits(p, expect(v, cfg, p_prev, m.grads(), b_prev, False, LR, s, muls, None)[0])
        m.close()
        runs.append(out)
    for a, bb in zip(*runs):
        assert same_bits(a[0], bb[0]) and same_bits(a[1], bb[1]) and same_bits(a[2], bb[2]) and a[3] == bb[3]


# ------------------------------------------------------------------ 4. the early per-chunk path
@pytest.mark.parametrize("nmb", [1, 2])
@pytest.mark.parametrize("prec", ["bf16", "fp8"])
def test_early_path_equals_one_pass(gpu, prec, nmb):
    """the per-chunk launches beside the backward (early_sgd 1) write the bits of the whole-arena launch
    (early_sgd 0): parameters, buffer, EMA and loss; the count advances once per step either way"""
    v = gpu
    cfg = setup(v, prec)[0]
    s = NESTEROV
    runs = []
    for early in (0, 1):
        m = build(v, prec, nmb)
        m.set_option("early_sgd", early)
        m.set_ema(D)
        m.set_sgd(*s)
        p, b, e = m.params(), None, m.ema()
        out = []
        v.kernel_hits_reset()
        for k in range(3):
            m.train_step(LR)
            m.sync()
            p, b = expect(v, cfg, p, m.grads(), b, k == 0, LR, s)
            e = v.ema.ema_ref(e, p, D)
            assert same_bits(m.params(), p) and same_bits(m.momentum(), b) and same_bits(m.ema(), e), (early, k)
            out.append((p, b, e, float(v.lib().vit_trainer_mean_loss(m.h))))
        hits = int(v.kernel_hits()[v.HIT_SGDM])
        assert m.sgd_info()["steps"] == 3
        m.close()
        assert hits == 3 * (cfg.num_layers + 2 if early else 1)  # one launch per gradient chunk / per step
        runs.append(out)
    for a, bb in zip(*runs):
        assert same_bits(a[0], bb[0]) and same_bits(a[1], bb[1]) and same_bits(a[2], bb[2]) and a[3] == bb[3]


# ------------------------------------------------------------------ 5. the unused path
@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp8"])
def test_unused_path_is_unchanged(gpu, prec, tmp_path):
    v = gpu
    cfg = setup(v, prec)[0]
    never, zero = build(v, prec), build(v, prec)
    zero.set_sgd(0, 0, 0, False)
    v.kernel_hits_reset()
    for k in range(3):
        for m in (never, zero):
            one_step(m, k)
    assert v.kernel_hits()[v.HIT_SGDM] == 0
    assert same_bits(never.params(), zero.params())
    assert never.device_bytes() == zero.device_bytes()
    for m in (never, zero):
        assert m.sgd_info() == dict(momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, steps=0)
        with pytest.raises(v.VitError):
            m.momentum()
    # the checkpoint of a trainer that never used momentum: the size and the flag bits it always had
    a, b = tmp_path / "a.bin", tmp_path / "b.bin"
    zero.save_checkpoint(a)
    v.write_checkpoint(b, cfg, zero.params())
    assert a.read_bytes() == b.read_bytes()
    assert np.frombuffer(a.read_bytes()[:1024], np.int32)[10] == 0
    assert v.read_checkpoint_momentum(a, cfg) == (None, (0.0, 0.0, 0.0, False), 0)
    # turning momentum on allocates nothing; the first momentum step allocates the buffer, once
    bytes0 = zero.device_bytes()
    zero.set_sgd(*PLAIN)
    assert zero.device_bytes() == bytes0
    for k in range(2):
        one_step(zero, k)
        assert zero.device_bytes() == bytes0 + 4 * arena_elems(v, cfg)
    assert v.kernel_hits()[v.HIT_SGDM] >= 2
    never.close()
    zero.close()


# ------------------------------------------------------------------ 6. checkpoints
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_checkpoint_resume(gpu, prec, tmp_path):
    v = gpu
    cfg = setup(v, prec)[0]
    s = DAMPENED
    whole = build(v, prec)
    whole.set_sgd(*s)
    for k in range(3):
        one_step(whole, k)
    first = build(v, prec)
    first.set_sgd(*s)
    for k in range(2):
        one_step(first, k)
    path = tmp_path / "resume.bin"
    first.save_checkpoint(path)
    b_file, s_file, n_file = v.read_checkpoint_momentum(path, cfg)
    assert same_bits(b_file, first.momentum()) and n_file == 2
    assert tuple(F32(x) for x in s_file[:3]) == tuple(F32(x) for x in s[:3]) and s_file[3] is False
    assert same_bits(v.read_checkpoint(path, cfg)[0], first.params())
    assert len(path.read_bytes()) == 1024 + 2 * 4 * cfg.num_params()
    first.close()
    second = build(v, prec, seed=11)  # other weights, momentum never set: the file brings all of it
    second.load_checkpoint(path)
    assert second.sgd_info() == whole.sgd_info() | {"steps": 2}
    assert same_bits(second.momentum(), b_file)
    second.set_batch(*setup(v, prec)[4:])
    one_step(second, 2)
    assert same_bits(whole.params(), second.params()) and same_bits(whole.momentum(), second.momentum())
    assert second.sgd_info() == whole.sgd_info() and whole.sgd_info()["steps"] == 3
    # a file without the section: the count goes to 0 (the next momentum step seeds the buffer again) and the
    # setting stays
    plain = tmp_path / "plain.bin"
    p_other = v.data.init_params(cfg, "parity", seed=21)
    v.write_checkpoint(plain, cfg, p_other)
    second.load_checkpoint(plain)
    assert second.sgd_info() == whole.sgd_info() | {"steps": 0}
    with pytest.raises(v.VitError):
        second.momentum()
    one_step(second, 1)
    want_p, want_b = expect(v, cfg, p_other, second.grads(), None, True, LR, s)
    assert same_bits(second.params(), want_p) and same_bits(second.momentum(), want_b)
    whole.close()
    second.close()


# ------------------------------------------------------------------ 7. errors leave the previous setting
def test_errors_leave_the_previous_setting(gpu):
    v = gpu
    m = build(v, "bf16")
    with pytest.raises(v.VitError):
        m.momentum()
    bad = [dict(momentum=0.0, nesterov=True), dict(momentum=0.9, dampening=0.1, nesterov=True), dict(momentum=-0.1),
           dict(momentum=float("nan")), dict(dampening=float("nan")), dict(weight_decay=-1e-4),
           dict(weight_decay=float("nan")), dict(momentum=INF), dict(momentum=0.0, weight_decay=5e-4)]
    for kw in bad:
        with pytest.raises(v.VitError):
            m.set_sgd(**kw)
    with pytest.raises(v.VitError, match="weight_decay"):
        m.set_sgd(momentum=0.0, weight_decay=5e-4)
    assert m.sgd_info() == dict(momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, steps=0)
    m.set_sgd(*DAMPENED)
    one_step(m, 0)
    before, b = m.sgd_info(), m.momentum()
    for kw in bad:
        with pytest.raises(v.VitError):
            m.set_sgd(**kw)
    assert m.sgd_info() == before and before["steps"] == 1 and same_bits(m.momentum(), b)
    m.set_ema(D)
    with m.ema_weights():
        with pytest.raises(v.VitError, match="EMA weights"):
            m.set_sgd(*PLAIN)
    assert m.sgd_info() == before
    # off keeps the buffer and the count; plain steps do not touch them; on again continues from them
    p = m.params()
    m.set_sgd(0, 0, 0, False)
    bytes_on = m.device_bytes()
    one_step(m, 1)
    assert same_bits(m.momentum(), b) and m.sgd_info()["steps"] == 1 and m.device_bytes() == bytes_on
    assert same_bits(m.params(), (p - (F32(LR) * m.grads()).astype(F32)).astype(F32))
    m.set_sgd(*DAMPENED)
    p = m.params()
    one_step(m, 1)
    want_p, want_b = expect(v, m.cfg, p, m.grads(), b, False, LR, DAMPENED)
    assert same_bits(m.params(), want_p) and same_bits(m.momentum(), want_b) and m.sgd_info()["steps"] == 2
    # lr = 0: the values stay, the buffer and the count advance; set_params does not touch the buffer
    p, b = m.params(), m.momentum()
    m.train_step(0.0)
    m.sync()
    assert same_bits(m.params(), p) and not same_bits(m.momentum(), b) and m.sgd_info()["steps"] == 3
    b = m.momentum()
    m.set_params(setup(v, "bf16", seed=9)[3])
    assert same_bits(m.momentum(), b) and m.sgd_info()["steps"] == 3
    m.close()


# ------------------------------------------------------------------ 8. interleaving with AdamW
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_interleaved_with_adamw(gpu, prec):
    v = gpu
    cfg = setup(v, prec)[0]
    s = NESTEROV
    m = build(v, prec)
    m.set_sgd(*s)
    p = m.params()
    one_step(m, 0)
    p, b = expect(v, cfg, p, m.grads(), None, True, LR, s)
    assert same_bits(m.params(), p) and same_bits(m.momentum(), b)
    fwd_bwd(m)
    m.optimizer_step_adamw(ALR, **HP)
    m.sync()
    m1, v1, t1 = m.adamw_state()
    assert t1 == 1 and same_bits(m.momentum(), b) and m.sgd_info()["steps"] == 1
    p = m.params()
    one_step(m, 1)
    p, b = expect(v, cfg, p, m.grads(), b, False, LR, s)
    assert same_bits(m.params(), p) and same_bits(m.momentum(), b) and m.sgd_info()["steps"] == 2
    m2, v2, t2 = m.adamw_state()
    assert t2 == 1 and same_bits(m1, m2) and same_bits(v1, v2)
    m.close()
