"""LAMB on the GPU (include/vit_trainer.h vit_trainer_step_lamb, include/vit_ops.h lamb_step)
against tests/lamb_ref.py, in stages like tests/test_gpu_gradclip.py: m and v bit-exact; |w| and |u| within one
fp32 ulp of the float64 numpy value (the device's double sum differs from numpy's by at most n * 2^-52
relative, so the rounded square root can differ only at a rounding boundary); the ratio bit-exact from the
device's own norms; p', the EMA and (through a forward) the bf16 shadow bit-exact from the device's own
ratio.  The references are fed the device's own gradients."""
import numpy as np
import pytest

import lamb_ref as R
from test_gpu_param_groups import MULS, arm, bits, build, clip_coef, draw, fwd_bwd, same_bits, setup, slices

pytestmark = pytest.mark.gpu

F32 = np.float32
LR = 3e-3
HP = dict(beta1=0.9, beta2=0.95, eps=1e-6, weight_decay=0.05)
BOTH = R.ALWAYS_ADAPT | R.TRUST_CLIP


def kw(flags):
    return dict(always_adapt=bool(flags & R.ALWAYS_ADAPT), trust_clip=bool(flags & R.TRUST_CLIP))


def check_record(what, wn, un, r, ref, wd_e, flags):
    """the device's {wn, un, r} against the reference segment `ref`"""
    assert R.ulp_apart(wn, ref["wn"]) <= 1, (what, "wn", float(wn), float(ref["wn"]))
    assert R.ulp_apart(un, ref["un"]) <= 1, (what, "un", float(un), float(ref["un"]))
    want = R.ratio(wn, un, wd_e, flags)
    assert F32(r).view(np.uint32) == want.view(np.uint32), (what, "r", float(r), float(want))


# ------------------------------------------------------------------ 1. the op
class Dev:
    """p, g, m, v of n elements at `off` floats into guarded device buffers"""

    def __init__(self, v, n, off, seed, p=None, g=None, m=None, vv=None):
        rng = np.random.default_rng(seed)
        self.v, self.n, self.off = v, n, off
        tot = n + off + 5
        mk = lambda a, s: np.concatenate([np.full(off, 7.5, F32), a if a is not None else s, np.full(5, -3.25, F32)])
        self.h = {"p": mk(p, (rng.standard_normal(n) * 0.05).astype(F32)),
                  "g": mk(g, (rng.standard_normal(n) * 1e-3).astype(F32)),
                  "m": mk(m, np.zeros(n, F32)), "v": mk(vv, np.zeros(n, F32))}
        assert all(a.size == tot for a in self.h.values())
        self.d = {k: v.DeviceArray.from_numpy(a) for k, a in self.h.items()}
        self.info = v.DeviceArray.from_numpy(np.full(5, -1.0, F32))

    def ptr(self, k):
        return self.d[k].ptr + 4 * self.off

    def step(self, lr, t, flags=0, info=True, **hp):
        self.v.lamb_step(self.ptr("p"), self.ptr("g"), self.ptr("m"), self.ptr("v"), self.n, lr, t=t,
                         info=self.info if info else None, **hp, **kw(flags))

    def get(self, k):
        a = self.d[k].numpy()
        sl = slice(self.off, self.off + self.n)
        guard = np.ones(a.size, bool)
        guard[sl] = False
        assert same_bits(a[guard], self.h[k][guard]), f"{k}: written outside the tensor"
        return a[sl]

    def close(self):
        for a in list(self.d.values()) + [self.info]:
            a.free()


def op_steps(v, n, off, flags, hp, steps=3, info=True, **init):
    """`steps` op steps checked against the reference -> the final p"""
    d = Dev(v, n, off, seed=n + off, **init)
    p, m_, v_ = (d.get(k) for k in "pmv")
    g = d.get("g")
    for t in range(1, steps + 1):
        d.step(LR, t, flags, info, **hp)
        pp, mm, vv = (d.get(k) for k in "pmv")
        assert same_bits(d.get("g"), g)
        ref = R.lamb_segment(p, g, m_, v_, LR, hp["beta1"], hp["beta2"], hp["eps"], hp["weight_decay"], t, flags)
        assert same_bits(mm, ref["m"]) and same_bits(vv, ref["v"]), (n, off, t)
        if info:
            rec = d.info.numpy()
            assert same_bits(rec[3:], np.full(2, -1.0, F32))
            check_record((n, off, t), rec[0], rec[1], rec[2], ref, hp["weight_decay"], flags)
            assert same_bits(pp, R.apply(p, ref["u"], LR, rec[2])), (n, off, t)
            last = rec[:3].copy()
        p, m_, v_ = pp, mm, vv
    d.close()
    return p, (last if info else None)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 64, 4095, 4096, 4097, 3 * 4096 + 20])
def test_lamb_step_op(gpu, n, off):
    p_info, _ = op_steps(gpu, n, off, 0, HP, info=True)
    p_null, _ = op_steps(gpu, n, off, 0, HP, info=False)
    assert same_bits(p_info, p_null)


# ------------------------------------------------------------------ 2. the op's branches
def test_lamb_step_op_branches(gpu, oracle32):
    v, n = gpu, 4096 + 77
    rng = np.random.default_rng(5)
    z = np.zeros(n, F32)
    p0 = (rng.standard_normal(n) * 0.05).astype(F32)
    # p all zero: r = 1
    _, rec = op_steps(v, n, 0, R.ALWAYS_ADAPT, HP, steps=1, p=z)
    assert rec[0] == 0 and rec[1] > 0 and rec[2] == 1
    # g = m = v = 0, wd = 0, always adapt: un = 0 and r = 1
    hp0 = dict(HP, weight_decay=0.0)
    p1, rec = op_steps(v, n, 0, R.ALWAYS_ADAPT, hp0, steps=1, p=p0, g=z)
    assert rec[0] > 0 and rec[1] == 0 and rec[2] == 1 and same_bits(p1, p0)
    # wd = 0 without the flag: r = 1 and p' has the AdamW oracle's bits
    g0 = (rng.standard_normal(n) * 1e-3).astype(F32)
    p1, rec = op_steps(v, n, 0, 0, hp0, steps=1, p=p0, g=g0)
    o = oracle32
    po, mo, vo = o.arr(p0.copy()), o.arr(z.copy()), o.arr(z.copy())
    o.adamw_step(po, o.arr(g0), mo, vo, LR, HP["beta1"], HP["beta2"], HP["eps"], 0.0, 1)
    assert rec[2] == 1 and same_bits(p1, po)
    # ... with the flag the same tensor is adapted
    _, rec = op_steps(v, n, 0, R.ALWAYS_ADAPT, hp0, steps=1, p=p0, g=g0)
    assert rec[2] != 1
    # trust clip: wn / un > 1 -> 1; wn / un < 1 stays
    _, rec = op_steps(v, n, 0, R.TRUST_CLIP, HP, steps=1, p=p0 * F32(1e4), g=g0)
    assert rec[0] / rec[1] > 1 and rec[2] == 1
    _, free = op_steps(v, n, 0, 0, HP, steps=1, p=p0 * F32(1e-4), g=g0)
    _, rec = op_steps(v, n, 0, R.TRUST_CLIP, HP, steps=1, p=p0 * F32(1e-4), g=g0)
    assert 0 < free[2] < 1 and same_bits(rec, free)


def test_lamb_step_op_arguments(gpu):
    v = gpu
    d = Dev(v, 100, 0, seed=1)
    for bad in (dict(beta1=1.0), dict(beta2=-0.1), dict(eps=-1.0), dict(weight_decay=float("inf")), dict(t=0)):
        with pytest.raises(v.VitError):
            v.lamb_step(d.ptr("p"), d.ptr("g"), d.ptr("m"), d.ptr("v"), 100, LR, **bad)
    with pytest.raises(v.VitError):
        v.call("lamb_step", d.ptr("p"), d.ptr("g"), d.ptr("m"), d.ptr("v"), 100, LR, 0.9, 0.95, 1e-6, 0.0, 1, 4, None)
    with pytest.raises(v.VitError):
        v.lamb_step(d.ptr("p"), d.ptr("g"), d.ptr("m"), d.ptr("v"), 0, LR)
    assert same_bits(d.get("p"), d.h["p"][:100]) and same_bits(d.get("m"), d.h["m"][:100])
    d.close()


# ------------------------------------------------------------------ 3. the trainer
def lamb_run(v, m, cfg, flags=0, steps=3, hp=HP, lr_mul=None, wd_mul=None, clip=None, ema=None):
    """`steps` LAMB steps of m, every (tensor, layer) slice against the reference; -> [(p, m, v, info)]"""
    one = np.ones((20, cfg.num_layers), F32)
    lr_mul = one if lr_mul is None else lr_mul
    wd_mul = one if wd_mul is None else wd_mul
    used = np.zeros((20, cfg.num_layers), bool)
    p = m.params()
    try:
        m_, v_, t0 = m.adamw_state()
    except v.VitError:
        m_, v_, t0 = np.zeros_like(p), np.zeros_like(p), 0
    e = m.ema() if ema is not None else None
    out = []
    for t in range(t0 + 1, t0 + steps + 1):
        g = fwd_bwd(m)
        m.optimizer_step_lamb(LR, **hp, **kw(flags))
        c = None
        if clip is not None:
            c = clip_coef(clip, m.grad_norm())
            assert c < 1 or t > t0 + 1  # (armed on the first step's norm; later ones may fall under it)
        pp, (mm, vv, tt), info = m.params(), m.adamw_state(), m.lamb_info()
        assert tt == t and same_bits(m.grads(), g)
        want = np.empty_like(p)
        for ti, l, sl in slices(v, cfg):
            used[ti, l] = True
            lr_e, wd_e = R.group_hp(LR, lr_mul[ti, l]), R.group_hp(hp["weight_decay"], wd_mul[ti, l])
            wn, un, r = (info[k][ti, l] for k in ("w_norm", "u_norm", "ratio"))
            ref = R.lamb_segment(p[sl], g[sl], m_[sl], v_[sl], lr_e, hp["beta1"], hp["beta2"], hp["eps"], wd_e, t,
                                 flags, c=c, r=r)
            assert same_bits(mm[sl], ref["m"]) and same_bits(vv[sl], ref["v"]), (ti, l, t)
            check_record((ti, l, t), wn, un, r, ref, wd_e, flags)
            want[sl] = ref["p"]
        bad = int((bits(pp) != bits(want)).sum())
        assert bad == 0, (t, bad)
        # entries of unlayered tensors at l > 0 hold 0, 0, 1
        assert np.all(info["w_norm"][~used] == 0) and np.all(info["u_norm"][~used] == 0)
        assert np.all(info["ratio"][~used] == 1)
        if ema is not None:
            e = v.ema.ema_ref(e, pp, ema)
            assert same_bits(m.ema(), e), t
        out.append((pp, mm, vv, info))
        p, m_, v_ = pp, mm, vv
    return out


def same_run(a, b):
    for (p0, m0, v0, i0), (p1, m1, v1, i1) in zip(a, b):
        assert same_bits(p0, p1) and same_bits(m0, m1) and same_bits(v0, v1)
        assert i0["steps"] == i1["steps"]
        for k in ("w_norm", "u_norm", "ratio"):
            assert same_bits(i0[k], i1[k]), k
    return True


@pytest.mark.parametrize("flags", [0, BOTH])
@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp8"])
def test_trainer_three_steps(gpu, prec, flags):
    v = gpu
    cfg = setup(v, prec)[0]
    m = build(v, prec)
    with pytest.raises(v.VitError):
        m.lamb_info()
    out = lamb_run(v, m, cfg, flags)
    m.close()
    info = out[-1][3]
    assert info["steps"] == 3
    if not flags:  # the ratios did matter
        assert np.count_nonzero(info["ratio"] != 1) > 10


@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp8"])
def test_no_decay_no_flags_is_adamw(gpu, prec):
    v = gpu
    hp = dict(HP, weight_decay=0.0)
    a, b = build(v, prec), build(v, prec)
    for t in range(3):
        ga, gb = fwd_bwd(a), fwd_bwd(b)
        assert same_bits(ga, gb)
        a.optimizer_step_lamb(LR, **hp)
        b.optimizer_step_adamw(LR, **hp)
        (ma, va, ta), (mb, vb, tb) = a.adamw_state(), b.adamw_state()
        assert ta == tb == t + 1
        assert same_bits(a.params(), b.params()) and same_bits(ma, mb) and same_bits(va, vb)
    assert np.all(a.lamb_info()["ratio"] == 1)
    # the two kinds share one state: the next steps exchanged still agree
    fwd_bwd(a), fwd_bwd(b)
    a.optimizer_step_adamw(LR, **hp)
    b.optimizer_step_lamb(LR, **hp)
    assert same_bits(a.params(), b.params()) and a.adamw_state()[2] == b.adamw_state()[2] == 4
    a.close()
    b.close()


def test_grid_stride_over_tiles(gpu):
    """more tiles than a launch has workgroups (each takes several, in several segments; the slots are those
    of the global tile numbers) and segments of many tiles: test_gpu_param_groups.py's wide arena"""
    v = gpu
    cfg = v.data.VitCfg("groups_wide", img=32, patch=8, channels=256, num_layers=12, num_heads=4, num_classes=10)
    params = v.data.init_params(cfg, "parity", seed=5)
    px, lab = v.data.synthetic_batch(cfg, 2, seed=6)
    lr_mul, wd_mul = draw(cfg, 20)
    m = v.ViT.build(cfg, 2, v.VIT_BF16, params=params)
    m.set_batch(px, lab)
    m.set_param_groups(lr_mul, wd_mul)
    lamb_run(v, m, cfg, R.ALWAYS_ADAPT, steps=1, lr_mul=lr_mul, wd_mul=wd_mul)
    m.close()


# ------------------------------------------------------------------ 4. everything on at once
@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp8"])
def test_groups_clip_ema_together(gpu, prec):
    v = gpu
    cfg = setup(v, prec)[0]
    lr_mul, wd_mul = draw(cfg, 41)
    assert (lr_mul == 0).any() and (wd_mul == 0).any() and set(np.unique(lr_mul)) <= set(MULS)
    runs = []
    for fused in (1, 0):
        m = build(v, prec)
        mx, _ = arm(m, 0.5)
        m.set_param_groups(lr_mul, wd_mul)
        m.set_ema(0.9)
        m.set_option("ema_fused", fused)
        out = lamb_run(v, m, cfg, 0, lr_mul=lr_mul, wd_mul=wd_mul, clip=mx, ema=0.9)
        runs.append((out, m.ema()))
        m.close()
    assert same_run(runs[0][0], runs[1][0]) and same_bits(runs[0][1], runs[1][1])
    # lr_mul = 0: the values frozen, m and v advanced, the ratio still computed
    p0 = setup(v, prec)[3]
    pp, mm, vv, info = runs[0][0][-1]
    frozen = 0
    for ti, l, sl in slices(v, cfg):
        if lr_mul[ti, l] == 0:
            frozen += 1
            assert same_bits(pp[sl], p0[sl]) and np.count_nonzero(mm[sl]) and np.count_nonzero(vv[sl])
            assert info["w_norm"][ti, l] > 0 and info["u_norm"][ti, l] > 0
            if wd_mul[ti, l] != 0:
                assert info["ratio"][ti, l] == info["w_norm"][ti, l] / info["u_norm"][ti, l]
    assert frozen > 0


# ------------------------------------------------------------------ 5. low-precision copies
@pytest.mark.parametrize("prec", ["bf16", "fp8"])
def test_low_precision_copies_refreshed(gpu, prec):
    v = gpu
    cfg, B, p, params, px, lab = setup(v, prec)
    m = build(v, prec)
    fwd_bwd(m)
    m.optimizer_step_lamb(LR, **HP)
    m.sync()
    m.forward()
    got = m.logits()
    fresh = v.ViT.build(cfg, B, p, params=m.params())
    fresh.set_concurrency(True)
    fresh.forward(px, lab)
    want = fresh.logits()
    fresh.close()
    m.close()
    assert same_bits(got, want)


# ------------------------------------------------------------------ 6. determinism
@pytest.mark.parametrize("prec", ["bf16", "fp8"])
def test_two_runs_are_identical(gpu, prec):
    v = gpu
    cfg = setup(v, prec)[0]
    runs = []
    for _ in range(2):
        m = build(v, prec)
        runs.append(lamb_run(v, m, cfg, R.ALWAYS_ADAPT, steps=2))
        m.close()
    assert same_run(*runs)


@pytest.mark.parametrize("nmb, conc", [(1, True), (2, True), (1, False)])
def test_settings_do_not_matter(gpu, nmb, conc):
    """whatever issued the backward, the step is the reference's function of the gradients it finds"""
    v, prec = gpu, "bf16"
    cfg = setup(v, prec)[0]
    m = build(v, prec, nmb)
    m.set_concurrency(conc)
    lamb_run(v, m, cfg, 0, steps=2)
    m.close()


# ------------------------------------------------------------------ 7. checkpoints
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_checkpoint_resume(gpu, prec, tmp_path):
    v = gpu
    cfg = setup(v, prec)[0]
    whole = build(v, prec)
    want = lamb_run(v, whole, cfg, 0, steps=3)
    whole.close()
    first = build(v, prec)
    lamb_run(v, first, cfg, 0, steps=2)
    path = tmp_path / "lamb.bin"
    first.save_checkpoint(path)
    first.close()
    info = v.checkpoint_info(path)
    assert info["has_opt"] and info["step"] == 2
    second = build(v, prec)
    second.load_checkpoint(path)
    got = lamb_run(v, second, cfg, 0, steps=1)
    second.close()
    p0, m0, v0, _ = want[2]
    p1, m1, v1, _ = got[0]
    assert same_bits(p0, p1) and same_bits(m0, m1) and same_bits(v0, v1)


def test_checkpoint_without_lamb_is_unchanged(gpu, tmp_path):
    v, prec = gpu, "bf16"
    files = []
    for asked in (False, True):
        m = build(v, prec)
        if asked:
            with pytest.raises(v.VitError):
                m.lamb_info()
        fwd_bwd(m)
        m.optimizer_step_adamw(LR, **HP)
        path = tmp_path / f"c{int(asked)}.bin"
        m.save_checkpoint(path)
        m.close()
        files.append(path.read_bytes())
    assert files[0] == files[1]


# ------------------------------------------------------------------ 8. unused means unchanged
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_unused_means_unchanged(gpu, prec):
    v = gpu

    def adamw_only(m):
        out = []
        for _ in range(2):
            fwd_bwd(m)
            m.optimizer_step_adamw(LR, **HP)
            out.append((m.params(),) + m.adamw_state())
        return out

    never = build(v, prec)
    before = adamw_only(never)  # (in a process that has run LAMB already: the same comparison)
    will = build(v, prec)
    fwd_bwd(will)
    bytes0 = will.device_bytes()
    ref = build(v, prec)
    fwd_bwd(ref)
    assert bytes0 == ref.device_bytes()
    ref.optimizer_step_adamw(LR, **HP)
    will.optimizer_step_lamb(LR, **HP)
    assert will.device_bytes() > ref.device_bytes()  # the tables, the slots and the records are counted
    assert never.device_bytes() == ref.device_bytes()
    will.close()
    ref.close()
    again = build(v, prec)
    after = adamw_only(again)
    for (p0, m0, v0, t0), (p1, m1, v1, t1) in zip(before, after):
        assert t0 == t1 and same_bits(p0, p1) and same_bits(m0, m1) and same_bits(v0, v1)
    never.close()
    again.close()


# ------------------------------------------------------------------ 9. errors
def test_errors_leave_the_state(gpu):
    v, prec = gpu, "bf16"
    m = build(v, prec)
    fwd_bwd(m)
    p0 = m.params()
    bad = [dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.5), dict(beta2=float("nan")), dict(eps=-1e-6),
           dict(eps=float("inf")), dict(weight_decay=-0.1), dict(weight_decay=float("nan"))]
    for b in bad:
        with pytest.raises(v.VitError):
            m.optimizer_step_lamb(LR, **dict(HP, **b))
    for flags in (4, -1, 1 << 16):
        assert v.lib().vit_trainer_step_lamb(m.h, LR, 0.9, 0.95, 1e-6, 0.05, flags) != 0
        with pytest.raises(v.VitError):
            v.check("step_lamb")
    with pytest.raises(v.VitError):
        m.lamb_info()
    with pytest.raises(v.VitError):
        m.adamw_state()  # nothing was allocated, t did not move
    assert same_bits(m.params(), p0)
    m.set_ema(0.9)
    with m.ema_weights():
        with pytest.raises(v.VitError, match="EMA weights in use"):
            m.optimizer_step_lamb(LR, **HP)
    assert same_bits(m.params(), p0)
    m.optimizer_step_lamb(LR, **HP)
    assert m.lamb_info()["steps"] == 1 and m.adamw_state()[2] == 1 and not same_bits(m.params(), p0)
    m.close()


# ------------------------------------------------------------------ 10. DP, world 1
@pytest.mark.parametrize("overlap", [True, False])
@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp8"])
def test_dp_world1_step(gpu, prec, overlap):
    v = gpu
    plain = build(v, prec)
    g0 = fwd_bwd(plain)
    plain.optimizer_step_lamb(LR, **HP)
    want = (plain.params(),) + plain.adamw_state()[:2] + (plain.lamb_info(),)
    plain.close()
    m = build(v, prec)
    m.dp_init(0, 1, v.ViT.dp_unique_id(), overlap=overlap)
    assert m.dp_ranks() == 1
    g = fwd_bwd(m)
    m.optimizer_step_lamb(LR, **HP)
    got = (m.params(),) + m.adamw_state()[:2] + (m.lamb_info(),)
    m.close()
    assert same_bits(g, g0) and same_run([want], [got])
