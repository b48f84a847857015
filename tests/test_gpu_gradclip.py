"""Global-norm gradient clipping on the GPU (include/vit_ops.h grad_sumsq, include/vit_trainer.h
vit_trainer_set_grad_clip / vit_trainer_grad_norm).

References: numpy float64 for the sum of squares, numpy fp32 (every operation rounded on its own)
for the clipped SGD update, the CPU oracle's ref_adamw_step fed the numpy-scaled gradients for the
clipped AdamW update, and trainers that never enabled clipping for the `c == 1` / unused paths.

Bounds.  Every square of an fp32 value is exact in double (48 significant bits), so the device sum
and numpy's differ only by the roundings of two differently ordered sums of n non-negative terms:
at most (n - 1) 2^-53 relative each, n 2^-52 together.  The fp32 norm is the rounding of the
square root of such a sum: one fp32 ulp is allowed for a result that lies at a rounding boundary.
The updates are bit-exact."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = float("inf")
LR = 0.01
PRECS = {"fp32": ("VIT_FP32", "test", 3), "bf16": ("VIT_BF16", "test_h64", 4), "fp8": ("VIT_FP8", "test_h64", 4)}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def norm_ref(g):
    return F32(np.sqrt((g.astype(np.float64) ** 2).sum()))


def ulps(a, b):
    """distance in fp32 ulps of two positive finite floats"""
    return abs(int(F32(a).view(np.int32)) - int(F32(b).view(np.int32)))


def check_norm(m, g, what=""):
    got, want = F32(m.grad_norm()), norm_ref(g)
    print(f"   grad_norm {what}: device {got!r} numpy {want!r} ({ulps(got, want)} ulp)")
    assert want > 0 and np.isfinite(want)
    assert ulps(got, want) <= 1, (what, got, want)
    return got


def clip_coef(max_norm, n):
    c = F32(max_norm) / (F32(n) + F32(1e-6))
    return c if c < F32(1.0) else F32(1.0)


def sgd_expect(p0, g, lr, c):
    """p - lr * (c * g), each operation rounded to fp32"""
    gs = (F32(c) * g).astype(F32)
    return (p0 - (F32(lr) * gs).astype(F32)).astype(F32)


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


def arm(m, frac=0.5):
    """One step with lr = 0 under max_norm = inf (p - 0 * g == p: the parameters, and so the next
    gradients, stay as they are) to read the norm, then max_norm = frac * norm: the clip is active
    in the step that follows without a magic number."""
    m.set_grad_clip(INF)
    m.train_step(0.0)
    m.sync()
    n0 = m.grad_norm()
    assert n0 > 0 and np.isfinite(n0)
    m.set_grad_clip(frac * n0)
    return frac * n0


# ------------------------------------------------------------------ the op
def sumsq(v, x, n, off=0):
    dx = v.DeviceArray.from_numpy(x if x.size else np.zeros(4, F32), F32)
    out = v.DeviceArray.from_numpy(np.array([-7.0]), np.float64)  # the op must overwrite it
    v.call("grad_sumsq", out, dx.ptr + 4 * off, n)
    first = out.numpy().copy()
    v.call("grad_sumsq", out, dx.ptr + 4 * off, n)
    return first, out.numpy().copy()


@pytest.mark.parametrize("n", [0, 1, 3, 63, 64, 65, 255, 4097, 2 ** 20 + 5])
def test_sumsq_op_vs_float64(gpu, n):
    v = gpu
    x = np.random.default_rng(100 + n).normal(size=n).astype(F32)
    got, _ = sumsq(v, x, n)
    ref = (x.astype(np.float64) ** 2).sum()
    if n == 0:
        assert got[0] == 0.0
        return
    err = abs(got[0] - ref) / ref
    print(f"\ngrad_sumsq n {n}: rel err {err:.3e} (bound {n * 2.0 ** -52:.3e})")
    assert err <= n * 2.0 ** -52, (got, ref)


@pytest.mark.parametrize("n,off", [(4097, 1), (4098, 2), (259, 3), (2, 1), (1, 3)])
def test_sumsq_op_unaligned_pointer(gpu, n, off):
    """a pointer that is not 16-byte aligned: the scalar head before the 16-byte loads"""
    v = gpu
    x = np.random.default_rng(7 * n + off).normal(size=n + off).astype(F32)
    got, _ = sumsq(v, x, n, off)
    ref = (x[off:].astype(np.float64) ** 2).sum()
    assert abs(got[0] - ref) / ref <= n * 2.0 ** -52, (got, ref)


@pytest.mark.parametrize("mag", [1e30, 1e-30])
def test_sumsq_op_extreme_magnitudes(gpu, mag):
    """squares of 1e30f overflow fp32 and squares of 1e-30f underflow it: any fp32 square or sum fails"""
    v = gpu
    n = 1000
    x = np.full(n, mag, F32)
    got, _ = sumsq(v, x, n)
    ref = (x.astype(np.float64) ** 2).sum()
    err = abs(got[0] - ref) / ref
    print(f"\ngrad_sumsq {mag:g} x {n}: got {got[0]:.17g} ref {ref:.17g} rel err {err:.3e}")
    assert np.isfinite(got[0]) and got[0] > 0
    assert err <= n * 2.0 ** -52, (got, ref)


def test_sumsq_op_is_deterministic(gpu):
    v = gpu
    n = 2 ** 20 + 5
    x = np.random.default_rng(5).normal(size=n).astype(F32)
    a, b = sumsq(v, x, n)
    assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ the norm, and c == 1
@functools.lru_cache(maxsize=None)
def unclipped_params(prec, nmb):
    """parameters after three steps of a trainer that never enabled clipping"""
    import vitpkg
    v = vitpkg.vit
    m = build(v, prec, nmb)
    for _ in range(3):
        m.train_step(LR)
    m.sync()
    p = m.params()
    m.close()
    p.setflags(write=False)
    return p


@pytest.mark.parametrize("ov", [0, 1])
@pytest.mark.parametrize("nmb", [1, 2, 4])
@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp8"])
def test_norm_matches_canonical_grads(gpu, prec, nmb, ov):
    v = gpu
    want = unclipped_params(prec, nmb)
    m = build(v, prec, nmb)
    m.set_option("clip_overlap", ov)
    assert m.grad_norm() == -1.0
    m.set_grad_clip(INF)
    print(f"\n{prec} nmb {nmb} clip_overlap {ov}")
    for k in range(3):
        m.train_step(LR)
        m.sync()
        check_norm(m, m.grads(), f"step {k}")
    p = m.params()
    m.close()
    assert same_bits(p, want)


# ------------------------------------------------------------------ the clipped updates
def clipped_sgd_step(m, max_norm, lr=LR):
    """zero_grad / forward / backward / step by hand; returns (g, p0, p1, expected p1, c)"""
    m.zero_grad()
    m.forward()
    m.backward()
    g, p0 = m.grads(), m.params()
    m.optimizer_step(lr)
    m.sync()
    n = check_norm(m, g, "clipped step")
    c = clip_coef(max_norm, n)
    return g, p0, m.params(), sgd_expect(p0, g, lr, c), c


@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp8"])
def test_clipped_sgd_is_bit_exact(gpu, prec):
    v = gpu
    m = build(v, prec)
    mx = arm(m)
    g, p0, p1, want, c = clipped_sgd_step(m, mx)
    print(f"\n{prec}: max_norm {mx!r} c {c!r}")
    assert c < 1
    bad = int((bits(p1) != bits(want)).sum())
    assert bad == 0, (bad, float(np.abs(p1 - want).max()))
    assert not same_bits(p1, sgd_expect(p0, g, LR, F32(1.0)))  # the clip did change the update
    assert same_bits(m.grads(), g)  # the arena is not scaled
    m.close()


HP = dict(beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.05)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_clipped_adamw_is_bit_exact(gpu, oracle32, prec):
    v, o = gpu, oracle32
    cfg, B, p, params, px, lab = setup(v, prec)
    m = build(v, prec)
    p_ref = o.arr(params)
    m_ref = o.arr(np.zeros_like(params))
    v_ref = o.arr(np.zeros_like(params))
    m.set_grad_clip(INF)
    cs = []
    for t in range(1, 4):
        m.zero_grad()
        m.forward()
        m.backward()
        g = m.grads()
        assert np.isfinite(g).all()
        mx = 0.5 * float(norm_ref(g))  # (set after the backward: the partial sums stay valid)
        m.set_grad_clip(mx)
        m.optimizer_step_adamw(3e-3, **HP)
        n = check_norm(m, g, f"adamw step {t}")
        c = clip_coef(mx, n)
        cs.append(c)
        o.adamw_step(p_ref, o.arr((c * g).astype(F32)), m_ref, v_ref, 3e-3, HP["beta1"], HP["beta2"], HP["eps"],
                     HP["weight_decay"], t)
        pp = m.params()
        mm, vv, tt = m.adamw_state()
        assert tt == t
        assert same_bits(mm, m_ref) and same_bits(vv, v_ref), t
        bad = int((bits(pp) != bits(p_ref)).sum())
        assert bad == 0, (t, bad, float(np.abs(pp - p_ref).max()))
    print(f"\n{prec} adamw: c per step {cs}")
    assert all(c < 1 for c in cs)
    m.close()


@pytest.mark.parametrize("early", [1, -1])
@pytest.mark.parametrize("prec", ["bf16", "fp8"])
def test_train_step_bypasses_early_sgd(gpu, prec, early):
    """the fused step under clipping (fp8's default takes the early per-chunk SGD without it) = the
    separate calls = the numpy statement"""
    v = gpu
    a, b = build(v, prec), build(v, prec)
    for m in (a, b):
        m.set_option("early_sgd", early)
    mx = arm(a)
    assert arm(b) == mx
    assert same_bits(a.params(), b.params())
    a.train_step(LR)
    a.sync()
    g, p0, p1, want, c = clipped_sgd_step(b, mx)
    assert c < 1
    assert same_bits(a.grads(), g)
    assert same_bits(p1, want)
    assert same_bits(a.params(), want)
    assert a.grad_norm() == b.grad_norm()
    a.close()
    b.close()


@pytest.mark.parametrize("prec", ["bf16", "fp8"])
def test_low_precision_copies_refreshed(gpu, prec):
    v = gpu
    cfg, B, p, params, px, lab = setup(v, prec)
    m = build(v, prec)
    arm(m)
    m.train_step(LR)
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


def three_clipped_steps(v, prec, nmb, ov):
    m = build(v, prec, nmb)
    m.set_option("clip_overlap", ov)
    mx = arm(m, 0.1)
    out = []
    for _ in range(3):
        m.train_step(LR)
        m.sync()
        out.append((float(v.lib().vit_trainer_mean_loss(m.h)), m.grads(), m.params(), m.grad_norm()))
        assert clip_coef(mx, out[-1][3]) < 1  # the clip stayed active
    m.close()
    return out


@pytest.mark.parametrize("nmb", [1, 2, 4])
@pytest.mark.parametrize("prec", ["bf16", "fp8"])
def test_overlapped_equals_plain(gpu, prec, nmb):
    v = gpu
    runs = [three_clipped_steps(v, prec, nmb, ov) for ov in (0, 1, 0, 1)]
    for other in runs[1:]:
        for (l0, g0, p0, n0), (l1, g1, p1, n1) in zip(runs[0], other):
            assert l0 == l1 and n0 == n1
            assert same_bits(g0, g1) and same_bits(p0, p1)


# ------------------------------------------------------------------ data parallel, world 1
@functools.lru_cache(maxsize=None)
def no_comm_clipped(prec):
    import vitpkg
    v = vitpkg.vit
    m = build(v, prec, seed=17)
    arm(m)
    m.train_step(LR)
    m.sync()
    out = (m.grads(), m.params(), m.grad_norm())
    m.close()
    return out


@pytest.mark.parametrize("overlap", [True, False])
@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp8"])
def test_dp_world1_clipped_step(gpu, prec, overlap):
    v = gpu
    g0, p0, n0 = no_comm_clipped(prec)
    m = build(v, prec, seed=17)
    m.dp_init(0, 1, v.ViT.dp_unique_id(), overlap=overlap)
    assert m.dp_ranks() == 1
    arm(m)
    m.train_step(LR)
    m.sync()
    g = m.grads()
    check_norm(m, g, f"dp overlap {overlap}")
    assert m.grad_norm() == n0
    assert same_bits(g, g0) and same_bits(m.params(), p0)
    m.close()


# ------------------------------------------------------------------ unused means unchanged
def three_steps(v, m, px, lab):
    m.set_batch(px, lab)
    m.sync()
    v.kernel_hits_reset()
    for _ in range(3):
        m.train_step(0.05)
    m.sync()
    hits = v.kernel_hits()
    return float(v.lib().vit_trainer_mean_loss(m.h)), m.grads(), m.params(), hits


@pytest.mark.parametrize("case", ["b_set_and_unset", "c_after_a_clipped_step"])
@pytest.mark.parametrize("prec", ["bf16", "fp8"])
def test_unused_means_unchanged(gpu, prec, case):
    v = gpu
    cfg, B, p, params, px, lab = setup(v, prec, seed=33)
    fresh = v.ViT.build(cfg, B, p, params=params)  # (a) never enabled
    want = three_steps(v, fresh, px, lab)
    fresh.close()
    m = v.ViT.build(cfg, B, p, params=params)
    if case == "b_set_and_unset":
        m.set_grad_clip(1.0)
        m.set_grad_clip(0.0)
    else:
        px2, lab2 = v.data.synthetic_batch(cfg, B, seed=35)
        m.set_grad_clip(1e-3)
        m.set_batch(px2, lab2)
        m.train_step(0.05)
        m.sync()
        m.set_grad_clip(0.0)
        m.set_params(params)
    got = three_steps(v, m, px, lab)
    m.close()
    assert got[0] == want[0]
    assert same_bits(got[1], want[1])
    assert same_bits(got[2], want[2])
    assert np.array_equal(got[3], want[3]), (np.nonzero(got[3] != want[3]), got[3], want[3])


# ------------------------------------------------------------------ arguments
def test_arguments_and_late_enable(gpu):
    v = gpu
    m = build(v, "bf16")
    assert m.grad_norm() == -1.0
    m.train_step(LR)  # an unclipped step computes no norm
    m.sync()
    assert m.grad_norm() == -1.0
    mx = arm(m)
    for bad in (-1.0, float("nan")):
        with pytest.raises(v.VitError):
            m.set_grad_clip(bad)
    # the previous setting (mx) is still in force, and enabling between backward and step works:
    # off during the backward (no partial sums issued), on again before the step
    m.set_grad_clip(0.0)
    m.zero_grad()
    m.forward()
    m.backward()
    g, p0 = m.grads(), m.params()
    m.set_grad_clip(mx)
    with pytest.raises(v.VitError):
        m.set_grad_clip(-2.0)
    m.optimizer_step(LR)
    m.sync()
    n = check_norm(m, g, "late enable")
    c = clip_coef(mx, n)
    assert c < 1
    assert same_bits(m.params(), sgd_expect(p0, g, LR, c))
    # ... and the setting kept across the failed calls clips the next fused step too
    g2, p2, p3, want, c2 = clipped_sgd_step(m, mx)
    assert c2 < 1 and same_bits(p3, want)
    m.close()
