"""EMA of the weights on the GPU (include/vit_trainer.h vit_trainer_set_ema): the stand-alone
ema_update op and the update fused into the optimizer kernels, against vit.ema.ema_ref (numpy fp32, each
product and the sum rounded on its own) fed with the device's own parameters.  Every comparison is bit-exact.

Shapes: CONFIGS["test"] with B = 3 in fp32 mode, CONFIGS["test_h64"] with B = 4 in bf16 / fp8 mode (the
fixtures of tests/test_gpu_param_groups.py, whose helpers the ones here follow)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = float("inf")
LR = 0.01
ALR = 3e-3
HP = dict(beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.05)
D = 0.9  # a small decay: the average moves visibly within three steps
PRECS = {"fp32": ("VIT_FP32", "test", 3), "bf16": ("VIT_BF16", "test_h64", 4), "fp8": ("VIT_FP8", "test_h64", 4)}
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


def arm(m, frac=0.1):
    """a norm-reading step at lr = 0 (the parameters stay), then max_norm = frac * norm: the clip stays active"""
    m.set_grad_clip(INF)
    m.train_step(0.0)
    m.sync()
    n0 = m.grad_norm()
    assert n0 > 0 and np.isfinite(n0)
    m.set_grad_clip(frac * n0)


def fwd_bwd(m):
    m.zero_grad()
    m.forward()
    m.backward()


def one_step(m, opt, k=1):
    """step k of a run: SGD through the separate calls first (k = 0), then through the fused train step"""
    if opt == "adamw":
        fwd_bwd(m)
        m.optimizer_step_adamw(ALR, **HP)
    elif k == 0:
        fwd_bwd(m)
        m.optimizer_step(LR)
    else:
        m.train_step(LR)
    m.sync()


def arena_elems(v, cfg):
    n = ctypes.c_longlong()
    assert v.lib().vit_layout_query(ctypes.byref(v._cfg_c(cfg)), None, None, ctypes.byref(n)) > 0
    return n.value


# ------------------------------------------------------------------ 1. the op
def op_values(n, seed):
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(F32)
    special = np.array([0.0, -0.0, 1e-45, -3e-42, 1.1754942e-38, -1e-38, 3e38, -2.5e38, 1e30, -65504.0], F32)
    k = min(n, special.size)
    a[rng.permutation(n)[:k]] = rng.permutation(special)[:k]
    return a


@pytest.mark.parametrize("offset", [0, 4])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4103, 2 ** 20 + 3])
def test_ema_update_op(gpu, n, offset):
    """float4 body + scalar tail; offset 4: a base that is 16-byte but not 64-byte aligned"""
    v = gpu
    e0, p0 = op_values(n + 2 * offset, n), op_values(n + 2 * offset, n + 1)
    assert n < 8 or ((e0 == 0).any() and (np.abs(p0[np.isfinite(p0)]) < 1e-38).any())
    pd = v.DeviceArray.from_numpy(p0)
    for d in (0.5, 0.999, 0.9999):
        ed = v.DeviceArray.from_numpy(e0)
        v.call("ema_update", ed.ptr + 4 * offset, pd.ptr + 4 * offset, n, d)
        got = ed.numpy()
        want = e0.copy()
        want[offset:offset + n] = v.ema.ema_ref(e0[offset:offset + n], p0[offset:offset + n], d)
        bad = np.nonzero(bits(got) != bits(want))[0]
        assert bad.size == 0, (d, bad[:8], got[bad[:8]], want[bad[:8]])  # (the elements around the range stay)
        ed.free()
    assert same_bits(pd.numpy(), p0)
    pd.free()


def test_ema_update_op_unaligned_and_counted(gpu):
    """a base that is not 16-byte aligned takes the scalar path; every call counts one HIT_EMA launch"""
    v = gpu
    n = 1029
    e0, p0 = op_values(n + 1, 5), op_values(n + 1, 6)
    ed, pd = v.DeviceArray.from_numpy(e0), v.DeviceArray.from_numpy(p0)
    v.kernel_hits_reset()
    v.call("ema_update", ed.ptr + 4, pd.ptr + 4, n, 0.999)
    v.call("ema_update", ed.ptr, pd.ptr, 0, 0.999)  # n = 0: nothing launched
    assert v.kernel_hits()[v.HIT_EMA] == 1
    want = e0.copy()
    want[1:] = v.ema.ema_ref(e0[1:], p0[1:], 0.999)
    assert same_bits(ed.numpy(), want)
    with pytest.raises(v.VitError):
        v.call("ema_update", ed.ptr, pd.ptr, n, 1.5)
    ed.free()
    pd.free()


# ------------------------------------------------------------------ 2. the recurrence, and no perturbation
@pytest.mark.parametrize("groups", [False, True], ids=["plain", "groups"])
@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("opt", ["sgd", "adamw"])
@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp8"])
def test_recurrence_and_no_perturbation(gpu, prec, opt, clip, groups):
    v = gpu
    cfg = setup(v, prec)[0]
    m, twin = build(v, prec), build(v, prec)  # the twin never enables EMA
    for t in (m, twin):
        if clip:
            arm(t)
        if groups:
            t.set_param_groups(*draw(cfg, 31))
    assert m.ema_info() == (0.0, 0, False)
    m.set_ema(D)
    d, u, on = m.ema_info()
    assert (F32(d), u, on) == (F32(D), 0, True)
    e = m.ema()
    assert same_bits(e, m.params())  # the seed
    p_start = m.params()
    for k in range(3):
        for t in (m, twin):
            one_step(t, opt, k)
        p = m.params()
        e = v.ema.ema_ref(e, p, D)
        got = m.ema()
        bad = int((bits(got) != bits(e)).sum())
        assert bad == 0, (k, bad, float(np.abs(got - e).max()))
        assert m.ema_info()[1] == k + 1
        if clip:
            assert m.grad_norm() > 0 and F32(m.grad_norm()) == F32(twin.grad_norm())
        # the training run itself is the twin's, bit for bit
        assert float(v.lib().vit_trainer_mean_loss(m.h)) == float(v.lib().vit_trainer_mean_loss(twin.h))
        assert same_bits(p, twin.params()) and same_bits(m.grads(), twin.grads())
        if opt == "adamw":
            (m1, v1, t1), (m2, v2, t2) = m.adamw_state(), twin.adamw_state()
            assert t1 == t2 == k + 1 and same_bits(m1, m2) and same_bits(v1, v2)
    assert not same_bits(p, p_start) and not same_bits(e, p)  # the weights moved and the average lags them
    with pytest.raises(v.VitError):
        twin.ema()
    m.close()
    twin.close()


# ------------------------------------------------------------------ 3. early SGD and micro-batches
@pytest.mark.parametrize("nmb", [1, 2, 4])
@pytest.mark.parametrize("prec", ["bf16", "fp8"])
def test_early_sgd_equals_one_pass(gpu, prec, nmb):
    """the per-chunk launches beside the backward (early_sgd 1) give the parameters and the average of the
    whole-arena pass (early_sgd 0), and both follow ema_ref"""
    v = gpu
    runs = []
    for early in (0, 1):
        m = build(v, prec, nmb)
        m.set_option("early_sgd", early)
        m.set_ema(D)
        e, out = m.ema(), []
        v.kernel_hits_reset()
        for _ in range(3):
            m.train_step(LR)
            m.sync()
            p = m.params()
            e = v.ema.ema_ref(e, p, D)
            assert same_bits(m.ema(), e), early
            out.append((p, e))
        hits = int(v.kernel_hits()[v.HIT_EMA])
        cfg = m.cfg
        m.close()
        assert hits == 3 * (cfg.num_layers + 2 if early else 1)  # one launch per gradient chunk / per step
        runs.append(out)
    for (p0, e0), (p1, e1) in zip(*runs):
        assert same_bits(p0, p1) and same_bits(e0, e1)


@pytest.mark.parametrize("opt", ["sgd", "adamw"])
@pytest.mark.parametrize("prec", ["bf16", "fp8"])
def test_unfused_option_same_bits(gpu, prec, opt):
    """option ema_fused = 0 (ema_update behind the optimizer kernels as they are without EMA; the form
    tools/bench_ema.py measures against) gives the bits of the fused kernels, with parameter groups too"""
    v = gpu
    cfg = setup(v, prec)[0]
    runs = []
    for fused in (1, 0):
        m = build(v, prec)
        m.set_option("ema_fused", fused)
        m.set_ema(D)
        out = []
        for k in range(3):
            if k == 2:
                m.set_param_groups(*draw(cfg, 33))
            one_step(m, opt, k)
            out.append((m.params(), m.ema()))
        m.close()
        runs.append(out)
    for (p0, e0), (p1, e1) in zip(*runs):
        assert same_bits(p0, p1) and same_bits(e0, e1)


# ------------------------------------------------------------------ 4. the decay is a per-step argument
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_decay_change_lr_zero_and_reseed(gpu, prec):
    v = gpu
    m = build(v, prec)
    m.set_ema(D)
    one_step(m, "sgd")
    e1 = m.ema()
    assert same_bits(e1, v.ema.ema_ref(setup(v, prec)[3], m.params(), D))
    d2 = v.ema.warmup_decay(0.9999, 1)
    m.set_ema(d2)  # only the decay changes: no re-seed, the count stays
    assert same_bits(m.ema(), e1) and m.ema_info()[1] == 1 and F32(m.ema_info()[0]) == F32(d2)
    one_step(m, "adamw")
    e2 = v.ema.ema_ref(e1, m.params(), d2)
    assert same_bits(m.ema(), e2) and m.ema_info()[1] == 2
    assert not same_bits(e2, v.ema.ema_ref(e1, m.params(), D))
    # a step at lr = 0 leaves the parameters and still averages
    p = m.params()
    m.train_step(0.0)
    m.sync()
    assert same_bits(m.params(), p)
    e3 = v.ema.ema_ref(e2, p, d2)
    assert same_bits(m.ema(), e3) and m.ema_info()[1] == 3 and not same_bits(e3, e2)
    # set_params does not touch the average
    m.set_params(setup(v, prec, seed=9)[3])
    assert same_bits(m.ema(), e3) and m.ema_info()[1] == 3
    # off keeps the buffer and stops the updates; the next switch on seeds it again
    bytes_on = m.device_bytes()
    m.set_ema(0)
    assert m.ema_info() == (0.0, 3, False)
    with pytest.raises(v.VitError):
        m.ema()
    one_step(m, "sgd")
    m.set_ema(0.5)
    assert m.device_bytes() == bytes_on
    assert same_bits(m.ema(), m.params()) and m.ema_info() == (0.5, 0, True)
    m.close()


# ------------------------------------------------------------------ 5. evaluating with the averaged weights
def _eval(m):
    pred, correct = m.evaluate()
    return pred, correct, m.logits()


@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp8"])
def test_ema_weights(gpu, prec, tmp_path):
    v = gpu
    cfg, B, p_enum, params, px, lab = setup(v, prec)
    m, twin = build(v, prec), build(v, prec)  # the twin does everything but enter the context
    rng = np.random.default_rng(7)
    arr = None
    for t in (m, twin):
        t.set_ema(D)
        for k in range(3):
            one_step(t, "sgd", k)
        if arr is None:
            arr = (t.ema() + 0.05 * rng.standard_normal(t.num_parameters)).astype(F32)
        t.set_ema_params(arr)
        assert same_bits(t.ema(), arr)
    live = m.params()
    pred0, correct0, logits0 = _eval(m)
    other = build(v, prec, params=arr)
    pred_a, correct_a, logits_a = _eval(other)
    other.close()
    assert not same_bits(logits_a, logits0)
    info = m.ema_info()
    grads = m.grads()
    with m.ema_weights() as inside:
        assert inside is m
        assert same_bits(m.params(), arr)
        pred, correct, logits = _eval(m)
        assert same_bits(logits, logits_a) and np.array_equal(pred, pred_a) and correct == correct_a
        m.forward()  # (a plain forward runs on them too)
        assert same_bits(m.logits(), logits_a)
        assert same_bits(m.ema(), arr)
        for call in (lambda: m.train_step(LR), m.backward, m.zero_grad, lambda: m.optimizer_step(LR),
                     lambda: m.optimizer_step_adamw(ALR, **HP), lambda: m.set_params(params),
                     lambda: m.save_checkpoint(tmp_path / "no.bin"), lambda: m.load_checkpoint(tmp_path / "no.bin"),
                     lambda: m.set_ema(0.5), lambda: m.set_ema(0), lambda: m.set_ema_params(params),
                     lambda: m._ok(v.lib().vit_trainer_ema_weights(m.h, 1), "enter twice")):
            with pytest.raises(v.VitError, match="EMA weights"):
                call()
        assert not (tmp_path / "no.bin").exists()
        assert m.ema_info() == info and same_bits(m.params(), arr) and same_bits(m.grads(), grads)
        assert same_bits(_eval(m)[2], logits_a)
    assert same_bits(m.params(), live) and same_bits(m.ema(), arr) and m.ema_info() == info
    pred, correct, logits = _eval(m)
    assert same_bits(logits, logits0) and np.array_equal(pred, pred0) and correct == correct0
    # the context leaves the mode however the block ends
    with pytest.raises(ZeroDivisionError):
        with m.ema_weights():
            1 / 0
    assert same_bits(m.params(), live)
    # ... and training goes on as if it had never been entered
    for t in (m, twin):
        t.evaluate()
        t.train_step(LR)
        t.sync()
    assert same_bits(m.params(), twin.params()) and same_bits(m.ema(), twin.ema())
    assert same_bits(m.ema(), v.ema.ema_ref(arr, m.params(), D)) and not same_bits(m.params(), live)
    m.close()
    twin.close()


def test_error_cases(gpu):
    v = gpu
    m = build(v, "bf16")
    L = v.lib()
    for call in (m.ema, lambda: m.set_ema_params(m.params()), lambda: m._ok(L.vit_trainer_ema_weights(m.h, 1), "enter"),
                 lambda: m._ok(L.vit_trainer_ema_weights(m.h, 0), "leave")):
        with pytest.raises(v.VitError):
            call()
    bytes0 = m.device_bytes()
    for bad in (float("nan"), -0.1, 1.0, 1.5, INF):
        with pytest.raises(v.VitError):
            m.set_ema(bad)
    assert m.ema_info() == (0.0, 0, False) and m.device_bytes() == bytes0
    m.set_ema(D)
    one_step(m, "sgd")
    e = m.ema()
    for bad in (float("nan"), -0.1, 1.0):
        with pytest.raises(v.VitError):
            m.set_ema(bad)
    d, u, on = m.ema_info()
    assert (F32(d), u, on) == (F32(D), 1, True) and same_bits(m.ema(), e)  # the previous setting stays
    with pytest.raises(v.VitError):
        m._ok(L.vit_trainer_ema_weights(m.h, 0), "leave while not in use")
    one_step(m, "sgd")
    assert same_bits(m.ema(), v.ema.ema_ref(e, m.params(), D))
    m.close()


# ------------------------------------------------------------------ 6. checkpoints
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_checkpoint_resume(gpu, prec, tmp_path):
    v = gpu
    cfg = setup(v, prec)[0]
    whole = build(v, prec)
    whole.set_ema(D)
    for _ in range(4):
        one_step(whole, "adamw")
    first = build(v, prec)
    first.set_ema(D)
    for _ in range(2):
        one_step(first, "adamw")
    path = tmp_path / "resume.bin"
    first.save_checkpoint(path)
    e_file, d_file, u_file = v.read_checkpoint_ema(path, cfg)
    assert same_bits(e_file, first.ema()) and F32(d_file) == F32(D) and u_file == 2
    assert same_bits(v.read_checkpoint(path, cfg)[0], first.params())
    first.close()
    second = build(v, prec, seed=11)  # other weights, EMA never set: the file brings all of it
    second.load_checkpoint(path)
    d, u, on = second.ema_info()
    assert (F32(d), u, on) == (F32(D), 2, True) and same_bits(second.ema(), e_file)
    second.set_batch(*setup(v, prec)[4:])
    for _ in range(2):
        one_step(second, "adamw")
    (m1, v1, t1), (m2, v2, t2) = whole.adamw_state(), second.adamw_state()
    assert t1 == t2 == 4 and same_bits(m1, m2) and same_bits(v1, v2)
    assert same_bits(whole.params(), second.params()) and same_bits(whole.ema(), second.ema())
    assert whole.ema_info() == second.ema_info() and second.ema_info()[1] == 4
    # a parameters-only file restarts the average of a trainer whose EMA is on
    p_other = v.data.init_params(cfg, "parity", seed=21)
    plain = tmp_path / "plain.bin"
    v.write_checkpoint(plain, cfg, p_other)
    second.load_checkpoint(plain)
    d, u, on = second.ema_info()
    assert (F32(d), u, on) == (F32(D), 0, True)
    assert same_bits(second.params(), p_other) and same_bits(second.ema(), p_other)
    # ... and leaves EMA off in a trainer that never had it on
    third = build(v, prec)
    third.load_checkpoint(plain)
    assert third.ema_info() == (0.0, 0, False)
    for t in (whole, second, third):
        t.close()


# ------------------------------------------------------------------ 7. the unused path
@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp8"])
def test_unused_path_is_unchanged(gpu, prec, tmp_path):
    """a trainer that never sets EMA: no EMA launch, the launch counters of the steps with EMA on differ from
    its own in the EMA entry alone (the fused form adds no launch in bf16 / fp8 mode; fp32-mode SGD adds its
    one ema_update, which is counted there and nowhere else), the memory it always allocated and the checkpoint
    bytes of the call without an EMA"""
    v = gpu
    cfg = setup(v, prec)[0]

    def two_steps(m):
        v.kernel_hits_reset()
        one_step(m, "sgd", 1)  # the fused train step (fp8: the early per-chunk path)
        one_step(m, "adamw")
        return v.kernel_hits()

    never, with_ema = build(v, prec), build(v, prec)
    two_steps(with_ema)  # (AdamW's m, v allocated in both before the memory is compared)
    h_never = two_steps(never)
    assert h_never[v.HIT_EMA] == 0
    assert never.device_bytes() == with_ema.device_bytes()
    bytes0 = with_ema.device_bytes()
    with_ema.set_ema(D)
    assert with_ema.device_bytes() == bytes0 + 4 * arena_elems(v, cfg)
    with_ema.set_ema(0.99)
    assert with_ema.device_bytes() == bytes0 + 4 * arena_elems(v, cfg)
    h_ema = two_steps(with_ema)
    h_never2 = two_steps(never)
    assert h_never2[v.HIT_EMA] == 0 and never.device_bytes() == bytes0
    want = h_never2.copy()  # (the same two steps of the same history)
    want[v.HIT_EMA] = (cfg.num_layers + 2 if prec == "fp8" else 1) + 1  # the SGD launch(es) + AdamW's
    assert np.array_equal(h_ema, want), np.nonzero(h_ema != want)
    # the checkpoint of the trainer without EMA: the bytes of the call that knows none
    a, b = tmp_path / "a.bin", tmp_path / "b.bin"
    never.save_checkpoint(a)
    mm, vv, t = never.adamw_state()
    v.write_checkpoint(b, cfg, never.params(), mm, vv, step=t, adamw=tuple(HP.values()))
    assert a.read_bytes() == b.read_bytes()
    assert v.read_checkpoint_ema(a, cfg) == (None, 0.0, 0)
    never.close()
    with_ema.close()
