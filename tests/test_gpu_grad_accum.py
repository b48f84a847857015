"""Gradient accumulation over micro-batches on the GPU (include/vit_trainer.h vit_trainer_set_grad_accum,
include/vit_ops.h grad_accumulate): the stand-alone op against numpy's fp32 `a + b`, a window
against vit.accum.accum_ref of the gradients a trainer without accumulation computes for the same micro-batches,
the accumulated gradient against the CPU oracle's one pass over the whole batch, and every optimizer step, the
fused train step and the world-1 all-reduce on top of the sum, against the references the existing tests use
for those steps.  Every comparison is bit-exact unless said otherwise.

Shapes: CONFIGS["test"] with B = 3 in fp32 mode, CONFIGS["test_h64"] with B = 4 in bf16 / fp8 mode (the
fixtures of tests/test_gpu_ema.py)."""
import functools

import numpy as np
import pytest

import lamb_ref as R
import parity
import test_gpu_param_groups as pg
import test_gpu_sgd_momentum as sm
from test_gpu_ema import D, arena_elems, bits, build, draw, op_values, same_bits, setup
from test_gpu_gradclip import check_norm, clip_coef, three_steps
from test_gpu_lamb import HP as LAMB_HP, LR as LAMB_LR, check_record
from test_gpu_model import oracle_step

pytestmark = pytest.mark.gpu

F32 = np.float32
LR = 0.01
N = 3          # micro-steps per window
SEED = 50      # micro-batch k of a window is synthetic_batch(seed = SEED + k)
LOWP = ["bf16", "fp8"]


def micro_batches(v, prec, n=N):
    cfg, B = setup(v, prec)[:2]
    return [v.data.synthetic_batch(cfg, B, seed=SEED + k) for k in range(n)]


@functools.lru_cache(maxsize=None)
def control(prec, nmb=None):
    """the gradients of the N micro-batches from a trainer with the same parameters and accumulation off:
    zero_grad / forward(b_global = N B) / backward per micro-batch.  Computed once per setting; read-only."""
    import vitpkg
    v = vitpkg.vit
    m = build(v, prec, nmb)
    out = []
    for px, lab in micro_batches(v, prec):
        m.zero_grad()
        m.forward(px, lab, b_global=N * m.B)
        m.backward()
        g = m.grads()
        g.setflags(write=False)
        out.append(g)
    assert m.grad_accum_info() == (1, 0)
    m.close()
    assert not same_bits(out[0], out[1]) and not same_bits(out[1], out[2])
    return tuple(out)


def micro_step(m, batch=None):
    """zero_grad + forward + backward of one micro-batch, nothing read back"""
    if batch is not None:
        m.set_batch(*batch)
    m.zero_grad()
    m.forward_async()  # b_global defaults to B * steps
    m.backward()


# ------------------------------------------------------------------ 1. the op
OFFSETS = [(0, 0, 0), (4, 4, 4), (1, 1, 1), (0, 1, 2)]
PAD = 8  # guard elements in front of and behind every range


def op_inputs(n, seed):
    """two buffers that hold a range of n elements at any offset of OFFSETS between two guards: op_values'
    finite values (zeros of both signs, denormals, 3e38-scale); no NaN and no inf, so no inf - inf"""
    size = n + 2 * PAD + 4
    a, b = op_values(size, seed), op_values(size, seed + 1)
    assert np.isfinite(a).all() and np.isfinite(b).all()
    return a, b


@pytest.mark.parametrize("offs", OFFSETS, ids=["aligned", "off4", "off1", "mixed"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4103, 2 ** 20 + 3])
def test_grad_accumulate_op(gpu, n, offs):
    """float4 body + scalar tail, the all-scalar path of a misaligned call, in place on either input; the
    elements around the range keep their bytes"""
    v = gpu
    a0, b0 = op_inputs(n, 7 * n)
    o0 = op_values(a0.size, 7 * n + 2)
    oo, oa, ob = (PAD + o for o in offs)
    if n >= 2:  # pairs that overflow, at the front of the range
        a0[oa:oa + 2] = [3e38, -3e38]
        b0[ob:ob + 2] = [3e38, -2.5e38]
    if n >= 16:  # sums that are +0, -0 and denormal, and a cancellation at the top of the range
        a0[oa + 2:oa + 8] = [0.0, -0.0, 1e-45, -3e-42, 1.1754942e-38, 3e38]
        b0[ob + 2:ob + 8] = [-0.0, -0.0, 1e-45, 1e-45, -1e-38, -2.5e38]
    with np.errstate(over="ignore"):
        want = (a0[oa:oa + n] + b0[ob:ob + n]).astype(F32)
    assert not np.isnan(want).any() and (n < 2 or (want[0] == np.inf and want[1] == -np.inf))
    if n >= 16:
        assert want[2] == 0 and not np.signbit(want[2]) and want[3] == 0 and np.signbit(want[3])
        assert all(0 < abs(x) < 1.1754942e-38 for x in want[4:7])
    for alias in ("separate", "out_is_a", "out_is_b"):
        da, db = v.DeviceArray.from_numpy(a0), v.DeviceArray.from_numpy(b0)
        do = v.DeviceArray.from_numpy(o0) if alias == "separate" else None
        pa, pb = da.ptr + 4 * oa, db.ptr + 4 * ob
        if alias == "separate":
            out_buf, out0, o_at = do, o0, oo
        elif alias == "out_is_a":
            out_buf, out0, o_at = da, a0, oa
        else:
            out_buf, out0, o_at = db, b0, ob
        v.grad_accumulate(out_buf.ptr + 4 * o_at, pa, pb, n)
        exp = out0.copy()
        exp[o_at:o_at + n] = want
        got = out_buf.numpy()
        bad = np.nonzero(bits(got) != bits(exp))[0]
        assert bad.size == 0, (alias, bad[:8], got[bad[:8]], exp[bad[:8]])
        # the inputs that are not the output are untouched
        if out_buf is not da:
            assert same_bits(da.numpy(), a0), alias
        if out_buf is not db:
            assert same_bits(db.numpy(), b0), alias
        for d in (da, db, do):
            if d is not None:
                d.free()


def test_grad_accumulate_op_counted_and_arguments(gpu):
    v = gpu
    n = 1029
    a0, b0 = op_inputs(n, 3)
    da, db, do = (v.DeviceArray.from_numpy(x) for x in (a0, b0, np.zeros_like(a0)))
    v.kernel_hits_reset()
    v.grad_accumulate(do, da, db, n)
    v.grad_accumulate(do.ptr + 4, da.ptr + 8, db, n)  # a misaligned call is one launch too
    v.grad_accumulate(do, da, db, 0)  # n = 0: nothing launched
    assert v.kernel_hits()[v.HIT_ACCUM] == 2
    for bad in (lambda: v.grad_accumulate(do, da, db, -1),
                lambda: v.grad_accumulate(da.ptr + 4, da, db, n),    # out overlaps a, one element along
                lambda: v.grad_accumulate(db.ptr + 4 * (n - 1), da, db, n),
                lambda: v.grad_accumulate(None, da, db, n)):
        with pytest.raises(v.VitError):
            bad()
    assert v.kernel_hits()[v.HIT_ACCUM] == 2
    assert same_bits(da.numpy(), a0) and same_bits(db.numpy(), b0)
    v.grad_accumulate(da.ptr + 4 * n, da, db, 4)  # exactly n apart is no overlap
    for d in (da, db, do):
        d.free()


# ------------------------------------------------------------------ 2. a window is the stated sum
WINDOW_CASES = [("fp32", None, 0)] + [(p, nmb, ov) for p in LOWP for nmb in (1, 2, 4) for ov in (0, 1)]


@pytest.mark.parametrize("prec, nmb, ov", WINDOW_CASES)
def test_window_is_the_stated_sum(gpu, prec, nmb, ov):
    v = gpu
    ctrl = control(prec, nmb)
    batches = micro_batches(v, prec)
    m = build(v, prec, nmb)
    if prec != "fp32":
        m.set_option("accum_overlap", ov)
    assert m.grad_accum_info() == (1, 0)
    bytes0 = m.device_bytes()
    m.set_grad_accum(N)
    assert m.grad_accum_info() == (N, 0) and m.device_bytes() == bytes0  # allocated by the first backward
    with pytest.raises(v.VitError):
        m.grad_accum()
    v.kernel_hits_reset()
    for k in range(1, N + 1):
        micro_step(m, batches[k - 1])
        assert m.grad_accum_info() == (N, k)
        if k < N:
            assert same_bits(m.grad_accum(), v.accum.accum_ref(ctrl[:k])), k
            assert same_bits(m.grads(), ctrl[k - 1]), k  # the micro-batch's own gradient
        else:
            assert same_bits(m.grads(), v.accum.accum_ref(ctrl))
            with pytest.raises(v.VitError):
                m.grad_accum()
    assert m.device_bytes() == bytes0 + 4 * arena_elems(v, m.cfg)
    chunks = m.cfg.num_layers + 2
    assert v.kernel_hits()[v.HIT_ACCUM] == (N - 1) * (chunks if ov else 1)  # (backward 1 is a copy)
    # two more windows back to back on the current batch with nothing read back in between: the next
    # micro-step's zero_grad and first writers follow the accumulate that reads the arena.  A backward while
    # the window is complete opens the next one.
    for _ in range(2 * N):
        micro_step(m)
    assert m.grad_accum_info() == (N, N)
    assert same_bits(m.grads(), v.accum.accum_ref([ctrl[N - 1]] * N))
    m.close()


# ------------------------------------------------------------------ 3. it is the big batch
def test_two_halves_are_the_whole_batch(gpu, oracle32):
    """fp32 mode: B = 3, N = 2 on the halves of a 6-image batch against the CPU oracle's gradient of all six in
    one pass, under the project's fp32 parity rule.  A wrong dloss scale shows here."""
    import oracle_ctypes as oc
    v = gpu
    cfg = v.data.CONFIGS["test"]
    params = v.data.init_params(cfg, "parity", seed=3)
    px, lab = v.data.synthetic_batch(cfg, 6, seed=SEED)
    loss_r, logits_r, g_r = oracle_step(oc, oracle32, cfg, params, px, lab, b_global=6)
    m = v.ViT.build(cfg, 3, v.VIT_FP32, params=params)
    m.set_grad_accum(2)
    losses, logits = [], []
    for h in range(2):
        m.zero_grad()
        losses.append(m.forward(px[3 * h:3 * h + 3], lab[3 * h:3 * h + 3]))  # b_global defaults to 3 * 2
        logits.append(m.logits())
        m.backward()
    g = m.grads()
    m.close()
    loss = float(np.mean(losses))
    print(f"\nloss {loss!r} oracle {loss_r!r} rel {abs(loss - loss_r) / abs(loss_r):.2e}")
    bad, rep = parity.check(parity.tensors(cfg, np.concatenate(logits), g, logits_r, g_r), parity.FP32)
    print(parity.summary(rep))
    assert not bad, bad
    assert abs(loss - loss_r) <= parity.FP32["loss"] * abs(loss_r)


# ------------------------------------------------------------------ 4. the step sees the sum, after it is final
def armed_trainer(v, prec, ov):
    """clipping armed, drawn parameter groups, the EMA on; then accumulation"""
    cfg = setup(v, prec)[0]
    m = build(v, prec)
    m.set_option("accum_overlap", ov)
    mx = sm.arm(m)
    muls = draw(cfg, 41)
    m.set_param_groups(*muls)
    m.set_ema(D)
    return m, cfg, mx, muls


def run_window(v, m, prec):
    for b in micro_batches(v, prec):
        micro_step(m, b)


@pytest.mark.parametrize("opt", ["sgd", "sgdm", "adamw", "lamb"])
@pytest.mark.parametrize("ov", [0, 1])
@pytest.mark.parametrize("prec", LOWP)
def test_step_sees_the_final_sum(gpu, oracle32, prec, ov, opt):
    v, o = gpu, oracle32
    m, cfg, mx, muls = armed_trainer(v, prec, ov)
    lr_mul, wd_mul = muls
    if opt == "sgdm":
        m.set_sgd(0.9, nesterov=True, weight_decay=5e-4)
    m.set_grad_accum(N)
    p0, e0 = m.params(), m.ema()
    run_window(v, m, prec)
    # the step right behind backward N, nothing read back before it
    if opt in ("sgd", "sgdm"):
        m.optimizer_step(LR)
    elif opt == "adamw":
        m.optimizer_step_adamw(pg.ALR, **pg.HP)
    else:
        m.optimizer_step_lamb(LAMB_LR, **LAMB_HP)
    m.sync()
    assert m.grad_accum_info() == (N, 0)
    g = m.grads()
    assert same_bits(g, v.accum.accum_ref(control(prec)))
    check_norm(m, g, f"{prec} accumulated, accum_overlap {ov}")
    c = clip_coef(mx, m.grad_norm())
    assert c < 1
    p = m.params()
    if opt == "sgd":
        want = pg.sgd_expect(v, cfg, p0, g, LR, lr_mul, c)
    elif opt == "sgdm":
        want, b = sm.expect(v, cfg, p0, g, None, True, LR, (0.9, 0.0, 5e-4, True), muls, c)
        assert same_bits(m.momentum(), b) and m.sgd_info()["steps"] == 1
    elif opt == "adamw":
        want, m_ref, v_ref = o.arr(p0.copy()), o.arr(np.zeros_like(p0)), o.arr(np.zeros_like(p0))
        pg.adamw_expect(v, o, cfg, want, g, m_ref, v_ref, pg.ALR, pg.HP["weight_decay"], lr_mul, wd_mul, 1, c)
        mm, vv, tt = m.adamw_state()
        assert tt == 1 and same_bits(mm, m_ref) and same_bits(vv, v_ref)
    else:
        want = np.empty_like(p0)
        (mm, vv, tt), info = m.adamw_state(), m.lamb_info()
        assert tt == 1
        zero = np.zeros_like(p0)
        for ti, l, sl in pg.slices(v, cfg):
            lr_e = R.group_hp(LAMB_LR, lr_mul[ti, l])
            wd_e = R.group_hp(LAMB_HP["weight_decay"], wd_mul[ti, l])
            wn, un, r = (info[k][ti, l] for k in ("w_norm", "u_norm", "ratio"))
            ref = R.lamb_segment(p0[sl], g[sl], zero[sl], zero[sl], lr_e, LAMB_HP["beta1"], LAMB_HP["beta2"],
                                 LAMB_HP["eps"], wd_e, 1, 0, c=c, r=r)
            assert same_bits(mm[sl], ref["m"]) and same_bits(vv[sl], ref["v"]), (ti, l)
            check_record((ti, l), wn, un, r, ref, wd_e, 0)
            want[sl] = ref["p"]
    bad = int((bits(p) != bits(want)).sum())
    assert bad == 0, (opt, bad, float(np.abs(p - want).max()))
    assert not same_bits(p, p0)
    assert same_bits(m.ema(), v.ema.ema_ref(e0, p, D)) and m.ema_info()[1] == 1
    m.close()


# ------------------------------------------------------------------ 5. train_step
@functools.lru_cache(maxsize=None)
def separate_calls_sgd(prec):
    """the parameters after one window through the separate calls and a plain SGD step"""
    import vitpkg
    v = vitpkg.vit
    m = build(v, prec)
    m.set_grad_accum(N)
    p0 = m.params()
    run_window(v, m, prec)
    m.optimizer_step(LR)
    m.sync()
    p = m.params()
    m.close()
    g = v.accum.accum_ref(control(prec))
    assert same_bits(p, (p0 - (F32(LR) * g).astype(F32)).astype(F32))
    p.setflags(write=False)
    return p


def train_step_window(v, prec, ov, early=None, check_mid=True):
    m = build(v, prec)
    m.set_option("accum_overlap", ov)
    if early is not None:
        m.set_option("early_sgd", early)
    m.set_grad_accum(N)
    p0 = m.params()
    for k, b in enumerate(micro_batches(v, prec), 1):
        m.set_batch(*b)
        m.train_step(LR)
        if k < N:
            assert m.grad_accum_info() == (N, k)
            if check_mid:
                assert same_bits(m.params(), p0), k
    m.sync()
    assert m.grad_accum_info() == (N, 0)
    p = m.params()
    assert not same_bits(p, p0)
    m.close()
    return p


@pytest.mark.parametrize("ov", [0, 1])
@pytest.mark.parametrize("prec", LOWP)
def test_train_step_window(gpu, prec, ov):
    v = gpu
    want = separate_calls_sgd(prec)
    assert same_bits(train_step_window(v, prec, ov), want)
    # ... and with nothing read back between the three calls
    assert same_bits(train_step_window(v, prec, ov, check_mid=False), want)
    if prec == "fp8":  # the early per-chunk SGD (fp8's default) runs in call 3 only, behind each chunk's sum
        assert same_bits(train_step_window(v, prec, ov, early=0, check_mid=False), want)
        assert same_bits(train_step_window(v, prec, ov, early=1, check_mid=False), want)


# ------------------------------------------------------------------ 6. data parallel, world 1
@functools.lru_cache(maxsize=None)
def no_comm_window(prec):
    import vitpkg
    v = vitpkg.vit
    return dp_window(v, prec, None)


def dp_window(v, prec, overlap):
    """a clipped window of three train_steps; overlap None: no communicator"""
    m = build(v, prec, seed=17)
    if overlap is not None:
        m.dp_init(0, 1, v.ViT.dp_unique_id(), overlap=overlap)
        assert m.dp_ranks() == 1
        m.set_option("dp_probe", 1)
    sm.arm(m)
    m.set_grad_accum(N)
    for b in micro_batches(v, prec):
        m.set_batch(*b)
        m.train_step(LR)
    m.sync()
    out = (m.grads(), m.params(), m.grad_norm(), m.dp_snapshot() if overlap is not None else None)
    assert m.grad_accum_info() == (N, 0)
    m.close()
    return out


@pytest.mark.parametrize("overlap", [True, False])
@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp8"])
def test_dp_world1_window(gpu, prec, overlap):
    v = gpu
    g0, p0, n0, _ = no_comm_window(prec)
    g, p, n, snap = dp_window(v, prec, overlap)
    assert same_bits(g, g0) and same_bits(p, p0) and n == n0
    assert not same_bits(p, setup(v, prec, seed=17)[3])
    # every chunk was summed before it was reduced: the snapshot taken behind each all-reduce is the sum
    cfg = setup(v, prec)[0]
    for (name, a), b in zip(cfg.split(snap).items(), cfg.split(g).values()):
        assert same_bits(a, b), name


# ------------------------------------------------------------------ 7. errors and state
def test_errors_and_state(gpu, tmp_path):
    v = gpu
    prec = "bf16"
    cfg = setup(v, prec)[0]
    m = build(v, prec)
    m.set_ema(D)
    m.set_sgd(0.9)
    m.set_grad_accum(N)
    micro_step(m)
    assert m.grad_accum_info() == (N, 1)
    p0, e0, bytes0, acc0 = m.params(), m.ema(), m.device_bytes(), m.grad_accum()
    for what, call in (("step", lambda: m.optimizer_step(LR)),
                       ("step_adamw", lambda: m.optimizer_step_adamw(pg.ALR, **pg.HP)),
                       ("step_lamb", lambda: m.optimizer_step_lamb(LAMB_LR, **LAMB_HP))):
        with pytest.raises(v.VitError, match="gradient accumulation: micro-step 1 of 3"):
            call()
        assert m.grad_accum_info() == (N, 1), what
        assert same_bits(m.params(), p0) and same_bits(m.ema(), e0) and m.ema_info()[1] == 0, what
        assert m.sgd_info()["steps"] == 0 and m.device_bytes() == bytes0, what  # (no m, v, buffer allocated)
        with pytest.raises(v.VitError):
            m.momentum()
    path = tmp_path / "mid.bin"
    with pytest.raises(v.VitError, match="gradient accumulation"):
        m.save_checkpoint(path)
    assert not path.exists()
    for bad in (0, -2):
        with pytest.raises(v.VitError):
            m.set_grad_accum(bad)
        assert m.grad_accum_info() == (N, 1) and m.accum_steps == N
    assert same_bits(m.grad_accum(), acc0)
    # a batch without labels does not count, and its backward fails without counting
    px, lab = setup(v, prec)[4:]
    m.set_batch(px, None)
    m.zero_grad()
    assert m.forward() == -1.0
    m.evaluate()
    assert m.grad_accum_info() == (N, 1) and same_bits(m.grad_accum(), acc0)
    with pytest.raises(v.VitError):
        m.backward()
    assert m.grad_accum_info() == (N, 1)
    m.set_batch(px, lab)
    # the way out of a window: any set call
    m.set_grad_accum(N)
    assert m.grad_accum_info() == (N, 0)
    with pytest.raises(v.VitError):
        m.grad_accum()
    m.save_checkpoint(path)  # no window open: as always
    assert path.exists()
    micro_step(m)
    micro_step(m)
    assert m.grad_accum_info() == (N, 2)
    m.load_checkpoint(path)
    assert m.grad_accum_info() == (N, 0) and same_bits(m.params(), p0)
    # a step with no window open runs as it always did
    micro_step(m)
    m.set_grad_accum(1)
    assert m.grad_accum_info() == (1, 0)
    m.optimizer_step(LR)
    m.sync()
    assert not same_bits(m.params(), p0) and m.sgd_info()["steps"] == 1
    assert m.device_bytes() == bytes0 + 4 * arena_elems(v, cfg)  # (the momentum buffer)
    m.close()


# ------------------------------------------------------------------ 8. unused means unchanged
@pytest.mark.parametrize("prec", LOWP)
def test_unused_means_unchanged(gpu, prec):
    v = gpu
    cfg, B, p, params, px, lab = setup(v, prec, seed=33)
    fresh = v.ViT.build(cfg, B, p, params=params)  # (a) never set
    want = three_steps(v, fresh, px, lab)
    bytes_a = fresh.device_bytes()
    assert want[3][v.HIT_ACCUM] == 0
    fresh.close()
    b = v.ViT.build(cfg, B, p, params=params)  # (b) set and unset
    b.set_grad_accum(N)
    b.set_grad_accum(1)
    c = v.ViT.build(cfg, B, p, params=params)  # (c) one full window run, then off and the parameters back
    c.set_grad_accum(N)
    v.kernel_hits_reset()
    for k in range(N):
        c.set_batch(*v.data.synthetic_batch(cfg, B, seed=35 + k))
        c.train_step(0.05)
    c.sync()
    assert v.kernel_hits()[v.HIT_ACCUM] > 0 and not same_bits(c.params(), params)
    c.set_grad_accum(1)
    c.set_params(params)
    for name, m in (("b", b), ("c", c)):
        got = three_steps(v, m, px, lab)
        assert m.device_bytes() == bytes_a + (4 * arena_elems(v, cfg) if name == "c" else 0)
        m.close()
        assert got[0] == want[0], name
        assert same_bits(got[1], want[1]) and same_bits(got[2], want[2]), name
        assert np.array_equal(got[3], want[3]), (name, np.nonzero(got[3] != want[3]), got[3], want[3])
