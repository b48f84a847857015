"""Parameter groups on the GPU (include/vit_trainer.h vit_trainer_set_param_groups):
per-(tensor, layer) multipliers of lr and weight decay inside the fused optimizer kernels.

References: the CPU oracle's ref_adamw_step called per (tensor, layer) slice of the canonical arrays
with fp32(lr * lr_mul) and fp32(wd * wd_mul), numpy fp32 (every operation rounded on its own) for
SGD, and trainers that never set groups.  Every comparison is bit-exact: the grouped kernels call the
ungrouped element updates with lr_e / wd_e, and the device's own gradients feed the references."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = float("inf")
LR = 0.01
ALR = 3e-3
HP = dict(beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.05)
PRECS = {"fp32": ("VIT_FP32", "test", 3), "bf16": ("VIT_BF16", "test_h64", 4), "fp8": ("VIT_FP8", "test_h64", 4)}
# non-powers of two and zero included
MULS = np.array([0.0, 0.25, 0.65, 0.65 ** 2, 1.0, 1.5], F32)


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


def build(v, prec, nmb=None, seed=3):
    cfg, B, p, params, px, lab = setup(v, prec, seed)
    m = v.ViT.build(cfg, B, p, params=params)
    m.set_concurrency(True)
    if nmb is not None:
        m.set_option("microbatch", nmb)
    m.set_batch(px, lab)
    return m


def draw(cfg, seed):
    """(lr_mul, wd_mul) [20, L], one draw of MULS per (tensor, layer)"""
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


def clip_g(g, c):
    """g' = c * g rounded to fp32 on its own (c None: no clipping)"""
    return g if c is None else (F32(c) * g).astype(F32)


def sgd_expect(v, cfg, p0, g, lr, lr_mul, c=None):
    """p - fp32(fp32(lr * lr_mul) * g') per (tensor, layer)"""
    out = np.empty_like(p0)
    gs = clip_g(g, c)
    for ti, l, sl in slices(v, cfg):
        lr_e = F32(F32(lr) * lr_mul[ti, l])
        out[sl] = (p0[sl] - (lr_e * gs[sl]).astype(F32)).astype(F32)
    return out


def adamw_expect(v, o, cfg, p_ref, g, m_ref, v_ref, lr, wd, lr_mul, wd_mul, t, c=None):
    """the oracle's AdamW per (tensor, layer) slice, in place on p_ref / m_ref / v_ref"""
    gs = o.arr(clip_g(g, c))
    for ti, l, sl in slices(v, cfg):
        lr_e = float(F32(F32(lr) * lr_mul[ti, l]))
        wd_e = float(F32(F32(wd) * wd_mul[ti, l]))
        o.adamw_step(p_ref[sl], gs[sl], m_ref[sl], v_ref[sl], lr_e, HP["beta1"], HP["beta2"], HP["eps"], wd_e, t)


def clip_coef(max_norm, n):
    c = F32(max_norm) / (F32(n) + F32(1e-6))
    return c if c < F32(1.0) else F32(1.0)


def arm(m, frac=0.5):
    """a norm-reading step at lr = 0 (the parameters stay), then max_norm = frac * norm"""
    m.set_grad_clip(INF)
    m.train_step(0.0)
    m.sync()
    n0 = m.grad_norm()
    assert n0 > 0 and np.isfinite(n0)
    m.set_grad_clip(frac * n0)
    return frac * n0, n0


def fwd_bwd(m):
    m.zero_grad()
    m.forward()
    m.backward()
    g = m.grads()
    assert np.isfinite(g).all()
    return g


def adamw_run(v, o, m, cfg, params, lr_mul, wd_mul, steps=3, clip=None):
    """`steps` AdamW steps of m against the per-slice oracle; every step bit-exact in p, m, v"""
    p_ref, m_ref, v_ref = o.arr(params.copy()), o.arr(np.zeros_like(params)), o.arr(np.zeros_like(params))
    for t in range(1, steps + 1):
        g = fwd_bwd(m)
        m.optimizer_step_adamw(ALR, **HP)
        c = None
        if clip is not None:
            c = clip_coef(clip, m.grad_norm())
            assert c < 1
        adamw_expect(v, o, cfg, p_ref, g, m_ref, v_ref, ALR, HP["weight_decay"], lr_mul, wd_mul, t, c)
        pp = m.params()
        mm, vv, tt = m.adamw_state()
        assert tt == t
        for what, got, want in (("p", pp, p_ref), ("m", mm, m_ref), ("v", vv, v_ref)):
            bad = int((bits(got) != bits(want)).sum())
            assert bad == 0, (what, t, bad, float(np.abs(got - want).max()))
    return p_ref


# ------------------------------------------------------------------ 1. AdamW vs the oracle
@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp8"])
def test_adamw_matches_per_slice_oracle(gpu, oracle32, prec):
    v = gpu
    cfg, B, p, params, px, lab = setup(v, prec)
    lr_mul, wd_mul = draw(cfg, 11)
    m = build(v, prec)
    m.set_param_groups(lr_mul, wd_mul)
    p3 = adamw_run(v, oracle32, m, cfg, params, lr_mul, wd_mul)
    m.close()
    # the groups did change the update: the ungrouped oracle differs
    q, mq, vq = (oracle32.arr(params.copy()), oracle32.arr(np.zeros_like(params)),
                 oracle32.arr(np.zeros_like(params)))
    assert not same_bits(p3, params)
    one = np.ones_like(lr_mul)
    m2 = build(v, prec)
    adamw_expect(v, oracle32, cfg, q, fwd_bwd(m2), mq, vq, ALR, HP["weight_decay"], one, one, 1)
    m2.close()
    assert not same_bits(q, p3)


# ------------------------------------------------------------------ 2. SGD vs numpy
@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp8"])
def test_sgd_matches_numpy(gpu, prec):
    v = gpu
    cfg, B, p, params, px, lab = setup(v, prec)
    lr_mul, _ = draw(cfg, 12)
    m = build(v, prec)
    m.set_param_groups(lr_mul=lr_mul)
    # separate calls
    g = fwd_bwd(m)
    p0 = m.params()
    m.optimizer_step(LR)
    m.sync()
    p1 = m.params()
    want = sgd_expect(v, cfg, p0, g, LR, lr_mul)
    assert same_bits(p1, want), int((bits(p1) != bits(want)).sum())
    assert not same_bits(p1, sgd_expect(v, cfg, p0, g, LR, np.ones_like(lr_mul)))
    assert same_bits(m.grads(), g)
    # the fused step
    m.train_step(LR)
    m.sync()
    assert same_bits(m.params(), sgd_expect(v, cfg, p1, m.grads(), LR, lr_mul))
    m.close()


@pytest.mark.parametrize("nmb", [1, 2])
@pytest.mark.parametrize("prec", ["bf16", "fp8"])
def test_early_sgd_equals_one_pass(gpu, prec, nmb):
    """the per-chunk launches of the grouped kernel (tile sub-ranges, beside the backward) give the
    bits of the whole-arena launch, and both are the numpy statement"""
    v = gpu
    cfg, B, p, params, px, lab = setup(v, prec)
    lr_mul, _ = draw(cfg, 13)
    runs = []
    for early in (0, 1):
        m = build(v, prec, nmb)
        m.set_option("early_sgd", early)
        m.set_param_groups(lr_mul=lr_mul)
        prev, out = m.params(), []
        for _ in range(3):
            m.train_step(LR)
            m.sync()
            g, pp = m.grads(), m.params()
            assert same_bits(pp, sgd_expect(v, cfg, prev, g, LR, lr_mul)), early
            out.append((g, pp))
            prev = pp
        m.close()
        runs.append(out)
    for (g0, p0), (g1, p1) in zip(*runs):
        assert same_bits(g0, g1) and same_bits(p0, p1)


# ------------------------------------------------------------------ 3. all ones == never set
def three_steps(v, m, opt):
    out = []
    for _ in range(3):
        if opt == "sgd":
            m.train_step(LR)
        else:
            fwd_bwd(m)
            m.optimizer_step_adamw(ALR, **HP)
        m.sync()
        out.append((float(v.lib().vit_trainer_mean_loss(m.h)), m.grads(), m.params()))
    return out


@pytest.mark.parametrize("opt", ["sgd", "adamw"])
@pytest.mark.parametrize("prec", ["bf16", "fp8"])
def test_all_ones_equals_never_set(gpu, prec, opt):
    v = gpu
    cfg = setup(v, prec)[0]
    ones = np.ones((20, cfg.num_layers), F32)
    never = build(v, prec)
    want = three_steps(v, never, opt)
    never.close()
    a = build(v, prec)
    a.set_param_groups(ones, ones)
    assert a.param_groups()[2] is True
    b = build(v, prec)  # groups switched on, then off again
    b.set_param_groups(*draw(cfg, 14))
    b.set_param_groups(None, None)
    lr_b, wd_b, on_b = b.param_groups()
    assert on_b is False and np.array_equal(lr_b, ones) and np.array_equal(wd_b, ones)
    for m in (a, b):
        got = three_steps(v, m, opt)
        m.close()
        for (l0, g0, p0), (l1, g1, p1) in zip(want, got):
            assert l0 == l1
            assert same_bits(g0, g1) and same_bits(p0, p1)


# ------------------------------------------------------------------ 4. with the clip active
@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp8"])
def test_clipped_sgd_with_groups(gpu, prec):
    v = gpu
    cfg = setup(v, prec)[0]
    lr_mul, _ = draw(cfg, 15)
    m = build(v, prec)
    mx, n0 = arm(m)  # n0: the norm this trainer reports without groups
    m.set_param_groups(lr_mul=lr_mul)
    g = fwd_bwd(m)
    p0 = m.params()
    m.optimizer_step(LR)
    m.sync()
    assert F32(m.grad_norm()).view(np.uint32) == F32(n0).view(np.uint32)  # the norm ignores the groups
    c = clip_coef(mx, m.grad_norm())
    assert c < 1
    assert same_bits(m.params(), sgd_expect(v, cfg, p0, g, LR, lr_mul, c))
    assert not same_bits(m.params(), sgd_expect(v, cfg, p0, g, LR, lr_mul))
    # the fused step (no early SGD under clipping)
    p1 = m.params()
    m.train_step(LR)
    m.sync()
    c = clip_coef(mx, m.grad_norm())
    assert c < 1
    assert same_bits(m.params(), sgd_expect(v, cfg, p1, m.grads(), LR, lr_mul, c))
    m.close()


@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp8"])
def test_clipped_adamw_with_groups(gpu, oracle32, prec):
    v = gpu
    cfg, B, p, params, px, lab = setup(v, prec)
    lr_mul, wd_mul = draw(cfg, 16)
    m = build(v, prec)
    mx, n0 = arm(m, 0.1)  # (0.1: the clip stays active over the three steps)
    m.set_param_groups(lr_mul, wd_mul)
    adamw_run(v, oracle32, m, cfg, params, lr_mul, wd_mul, clip=mx)
    m.close()


# ------------------------------------------------------------------ 5. bf16 shadow and derived copies
@pytest.mark.parametrize("opt", ["sgd", "adamw"])
@pytest.mark.parametrize("prec", ["bf16", "fp8"])
def test_low_precision_copies_refreshed(gpu, prec, opt):
    v = gpu
    cfg, B, p, params, px, lab = setup(v, prec)
    m = build(v, prec)
    m.set_param_groups(*draw(cfg, 17))
    if opt == "sgd":
        m.train_step(LR)  # (fp8: the early per-chunk path)
    else:
        fwd_bwd(m)
        m.optimizer_step_adamw(ALR, **HP)
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


# ------------------------------------------------------------------ 6. freeze
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_freeze_all_but_the_head(gpu, prec):
    v = gpu
    cfg, B, p, params, px, lab = setup(v, prec)
    m = build(v, prec)
    m.set_param_groups(lr_mul={n: (1.0 if n in ("head_w", "head_b") else 0.0) for n in v.data.PARAM_NAMES})
    for _ in range(2):
        fwd_bwd(m)
        m.optimizer_step_adamw(ALR, **HP)
    m.sync()
    got, (mm, vv, t) = cfg.split(m.params()), m.adamw_state()
    m.close()
    ref, mm, vv = cfg.split(params), cfg.split(mm), cfg.split(vv)
    for n in v.data.PARAM_NAMES:
        if n in ("head_w", "head_b"):
            assert (bits(got[n]) != bits(ref[n])).mean() > 0.9, n
        else:
            assert same_bits(got[n], ref[n]), n  # frozen: not even weight decay moves it
            assert np.count_nonzero(mm[n]) > 0 and np.count_nonzero(vv[n]) > 0, n  # m, v still advance


# ------------------------------------------------------------------ 7. the recipe through the wrapper
def test_recipe_no_decay_and_layer_decay(gpu, oracle32):
    v = gpu
    prec = "bf16"
    cfg, B, p, params, px, lab = setup(v, prec)
    lr_mul, wd_mul = v.groups.layer_decay(cfg, 0.75), v.groups.no_decay(cfg)
    m = build(v, prec)
    m.set_param_groups(lr_mul=lr_mul, wd_mul=wd_mul)
    lr_got, wd_got, on = m.param_groups()
    assert on is True
    # (entries the library ignores read back as 1; compare the used ones)
    for ti, l, _ in slices(v, cfg):
        assert lr_got[ti, l] == lr_mul[ti, l] and wd_got[ti, l] == wd_mul[ti, l]
    adamw_run(v, oracle32, m, cfg, params, lr_mul, wd_mul)
    m.close()


# ------------------------------------------------------------------ 8. arguments
def test_arguments(gpu):
    v = gpu
    prec = "bf16"
    cfg = setup(v, prec)[0]
    names, L = v.data.PARAM_NAMES, cfg.num_layers
    ones = np.ones((20, L), F32)
    m = build(v, prec)
    lr0, wd0, on0 = m.param_groups()
    assert on0 is False and np.array_equal(lr0, ones) and np.array_equal(wd0, ones)
    lr_mul, wd_mul = draw(cfg, 18)
    # entries of l > 0 of the tensors outside the blocks are ignored: they may hold anything
    for n, junk in zip(("patch_w", "cls", "lnfb", "head_w"), (np.nan, -3.0, INF, -INF)):
        lr_mul[names.index(n), 1:] = junk
        wd_mul[names.index(n), 1:] = junk
    m.set_param_groups(lr_mul, wd_mul)
    kept_lr, kept_wd, on = m.param_groups()
    assert on is True
    used = np.zeros((20, L), bool)
    for ti, l, _ in slices(v, cfg):
        used[ti, l] = True
    assert np.array_equal(kept_lr[used], lr_mul[used]) and np.array_equal(kept_wd[used], wd_mul[used])
    assert np.all(kept_lr[~used] == 1) and np.all(kept_wd[~used] == 1)
    for bad in (np.nan, -0.5, INF):
        for which in ("lr", "wd"):
            t = ones.copy()
            t[names.index("fcw"), L - 1] = bad
            with pytest.raises(v.VitError):
                m.set_param_groups(t, None) if which == "lr" else m.set_param_groups(None, t)
            got_lr, got_wd, on = m.param_groups()
            assert on is True and np.array_equal(got_lr, kept_lr) and np.array_equal(got_wd, kept_wd)
    # ... and the next step still runs with the tables kept across the failed calls
    g = fwd_bwd(m)
    p0 = m.params()
    m.optimizer_step(LR)
    m.sync()
    assert same_bits(m.params(), sgd_expect(v, cfg, p0, g, LR, lr_mul))
    with pytest.raises(ValueError):
        m.set_param_groups(lr_mul={"no_such_tensor": 1.0})
    m.close()


# ------------------------------------------------------------------ 9. determinism
@pytest.mark.parametrize("prec", ["bf16", "fp8"])
def test_two_grouped_runs_are_identical(gpu, prec):
    v = gpu
    cfg = setup(v, prec)[0]
    runs = []
    for _ in range(2):
        m = build(v, prec)
        m.set_param_groups(*draw(cfg, 19))
        out = three_steps(v, m, "sgd") + three_steps(v, m, "adamw")
        m.close()
        runs.append(out)
    for (l0, g0, p0), (l1, g1, p1) in zip(*runs):
        assert l0 == l1 and same_bits(g0, g1) and same_bits(p0, p1)


# ------------------------------------------------------------------ more tiles than workgroups
def test_grid_stride_over_tiles(gpu, oracle32):
    """an arena of more tiles than a grouped launch has workgroups (each then takes several tiles,
    in several segments), and segments of many tiles: one SGD and one AdamW step against the
    references"""
    v = gpu
    cfg = v.data.VitCfg("groups_wide", img=32, patch=8, channels=256, num_layers=12, num_heads=4, num_classes=10)
    B = 2
    tiles = sum(-(-(((n // (cfg.num_layers if name in v.data.LAYER_PARAMS else 1)) + 63) // 64 * 64) // 4096)
                * (cfg.num_layers if name in v.data.LAYER_PARAMS else 1)
                for name, n in zip(v.data.PARAM_NAMES, cfg.param_sizes()))
    assert tiles > 2048, tiles
    params = v.data.init_params(cfg, "parity", seed=5)
    px, lab = v.data.synthetic_batch(cfg, B, seed=6)
    lr_mul, wd_mul = draw(cfg, 20)
    m = v.ViT.build(cfg, B, v.VIT_BF16, params=params)
    m.set_batch(px, lab)
    m.set_param_groups(lr_mul, wd_mul)
    m.train_step(LR)
    m.sync()
    p1 = m.params()
    assert same_bits(p1, sgd_expect(v, cfg, params, m.grads(), LR, lr_mul))
    adamw_run(v, oracle32, m, cfg, p1, lr_mul, wd_mul, steps=1)
    m.close()
