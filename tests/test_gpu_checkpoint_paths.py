"""The trainer's one save path and one load path (vit_trainer_save_checkpoint / _load_checkpoint)
over every reachable combination of optimizer state, and the counters of the three step calls.  The files are
compared with the numpy statement of the format (tests/ckpt_format.py) fed from the getters.  Every comparison is
on bits; no tolerance is involved.

Shapes: CONFIGS["test"] with B = 3 in fp32 mode, CONFIGS["test_h64"] with B = 4 in bf16 / fp8 mode (the
fixtures of tests/test_gpu_ema.py and tests/test_gpu_sgd_momentum.py)."""
import numpy as np
import pytest

import ckpt_format

pytestmark = pytest.mark.gpu

F32 = np.float32
LR, ALR = 0.01, 3e-3
HP = dict(beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.05)
LAMB_HP = dict(beta1=0.9, beta2=0.99, eps=1e-6, weight_decay=0.02)
D = 0.9
SGD = (0.9, 0.0, 5e-4, True)
PRECS = {"fp32": ("VIT_FP32", "test", 3), "bf16": ("VIT_BF16", "test_h64", 4), "fp8": ("VIT_FP8", "test_h64", 4)}
# the reachable states: (EMA on, momentum set, the steps that reach it)
CASES = {
    "none": (False, False, ("sgd",)),
    "adamw": (False, False, ("adamw", "adamw")),
    "lamb": (False, False, ("lamb", "lamb")),
    "ema": (True, False, ("sgd", "sgd")),
    "momentum": (False, True, ("sgd", "sgd")),
    "adamw_ema": (True, False, ("adamw", "adamw")),
    "momentum_ema": (True, True, ("sgd", "sgd")),
    "adamw_momentum_ema": (True, True, ("adamw", "sgd")),
}
# the state every file is loaded over: other settings than the cases', so that a kept one shows
FULL_D, FULL_SGD = 0.8, (0.8, 0.0, 0.0, False)


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


def build(v, prec, seed=3):
    cfg, B, p, params, _, _ = setup(v, prec, seed)
    m = v.ViT.build(cfg, B, p, params=params)
    m.set_concurrency(True)
    m.set_batch(*setup(v, prec)[4:])  # (the same batch whatever the weights' seed)
    return m


def step(m, kind, fused=False):
    """one real step: forward, backward and the optimizer call `kind` (sgd, fused: the fused train step)"""
    if kind == "sgd" and fused:
        m.train_step(LR)
    else:
        m.zero_grad()
        m.forward()
        m.backward()
        if kind == "sgd":
            m.optimizer_step(LR)
        elif kind == "adamw":
            m.optimizer_step_adamw(ALR, **HP)
        else:
            m.optimizer_step_lamb(ALR, **LAMB_HP)
    m.sync()


def run_case(m, case):
    ema, mom, steps = CASES[case]
    if ema:
        m.set_ema(D)
    if mom:
        m.set_sgd(*SGD)
    for k, kind in enumerate(steps):
        step(m, kind, fused=k > 0)
    return HP if "adamw" in steps else LAMB_HP if "lamb" in steps else None


def snapshot(v, m):
    """everything the getters return; None for a state that does not exist"""
    s = {"params": m.params(), "ema_info": m.ema_info(), "sgd_info": m.sgd_info(), "m": None, "v": None, "t": 0,
         "ema": None, "momentum": None}
    try:
        s["m"], s["v"], s["t"] = m.adamw_state()
    except v.VitError:
        pass
    if s["ema_info"][2]:
        s["ema"] = m.ema()
    try:
        s["momentum"] = m.momentum()
    except v.VitError:
        pass
    return s


def same_snapshot(a, b):
    for k in ("ema_info", "sgd_info", "t"):
        if a[k] != b[k]:
            return False
    for k in ("params", "m", "v", "ema", "momentum"):
        if (a[k] is None) != (b[k] is None) or (a[k] is not None and not same_bits(a[k], b[k])):
            return False
    return True


def statement(cfg, s, hp):
    """the file of a trainer in state s (a snapshot), by the numpy statement of the format"""
    kw = dict(params=s["params"])
    if s["m"] is not None:
        kw.update(m=s["m"], v=s["v"], step=s["t"], adamw=(hp["beta1"], hp["beta2"], hp["eps"], hp["weight_decay"]))
    if s["ema"] is not None:
        kw.update(ema=s["ema"], ema_decay=s["ema_info"][0], ema_updates=s["ema_info"][1])
    if s["momentum"] is not None:
        i = s["sgd_info"]
        kw.update(momentum=s["momentum"], sgd=(i["momentum"], i["dampening"], i["weight_decay"], i["nesterov"]),
                  momentum_steps=i["steps"])
    return ckpt_format.encode(cfg, **kw)


def full_trainer(v, prec):
    """a trainer with every state: AdamW stepped, EMA on, momentum stepped"""
    m = build(v, prec, seed=11)
    m.set_ema(FULL_D)
    m.set_sgd(*FULL_SGD)
    step(m, "adamw")
    step(m, "sgd")
    return m


@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp8"])
@pytest.mark.parametrize("case", list(CASES))
def test_save_and_load(gpu, prec, case, tmp_path):
    v = gpu
    cfg = setup(v, prec)[0]
    ema, mom, steps = CASES[case]
    first = build(v, prec)
    hp = run_case(first, case)
    s0 = snapshot(v, first)
    assert (s0["m"] is not None) == (hp is not None) and (s0["ema"] is not None) == ema
    assert (s0["momentum"] is not None) == mom

    # ---- save: the numpy statement's bytes
    path = tmp_path / "s.bin"
    first.save_checkpoint(path)
    raw = path.read_bytes()
    assert raw == statement(cfg, s0, hp)
    assert same_snapshot(snapshot(v, first), s0)  # (saving changes nothing)

    # ---- load into a fresh trainer: the same bits, counters and settings, and the same next steps
    second = build(v, prec, seed=11)
    second.load_checkpoint(path)
    assert same_snapshot(snapshot(v, second), s0)
    for m in (first, second):
        for kind in steps:
            step(m, kind, fused=True)
    s1 = snapshot(v, first)
    assert same_snapshot(snapshot(v, second), s1)
    assert not same_bits(s1["params"], s0["params"])
    first.close()
    second.close()

    # ---- a refused load changes nothing; then the load over existing state
    full = full_trainer(v, prec)
    f0 = snapshot(v, full)
    assert f0["m"] is not None and f0["ema"] is not None and f0["momentum"] is not None
    bad = tmp_path / "bad.bin"
    bad.write_bytes(raw[:-4])
    with pytest.raises(v.VitError):
        full.load_checkpoint(bad)
    other = v.data.CONFIGS["test" if cfg is v.data.CONFIGS["test_h64"] else "test_h64"]
    v.write_checkpoint(bad, other, v.data.init_params(other, "parity", seed=5))
    with pytest.raises(v.VitError, match="config differs"):
        full.load_checkpoint(bad)
    assert same_snapshot(snapshot(v, full), f0)
    full.load_checkpoint(path)
    f1 = snapshot(v, full)
    assert same_bits(f1["params"], s0["params"])
    if s0["m"] is not None:
        assert same_bits(f1["m"], s0["m"]) and same_bits(f1["v"], s0["v"]) and f1["t"] == s0["t"]
    else:  # a parameters-only file restarts AdamW
        assert not bits(f1["m"]).any() and not bits(f1["v"]).any() and f1["t"] == 0
    if s0["momentum"] is not None:
        assert same_bits(f1["momentum"], s0["momentum"]) and f1["sgd_info"] == s0["sgd_info"]
    else:  # the count goes to 0, the setting stays
        assert f1["momentum"] is None and f1["sgd_info"] == f0["sgd_info"] | {"steps": 0}
    if s0["ema"] is not None:
        assert same_bits(f1["ema"], s0["ema"]) and f1["ema_info"] == s0["ema_info"]
    else:  # the average starts again from the loaded parameters, the decay stays
        assert same_bits(f1["ema"], s0["params"]) and f1["ema_info"] == (f0["ema_info"][0], 0, True)
    full.close()


def lamb_steps(v, m):
    try:
        return m.lamb_info()["steps"]
    except v.VitError:
        return 0


# (HIT_EMA, HIT_SGDM, adam_t, LAMB steps, momentum steps, EMA updates) after three steps with the EMA and
# momentum on, bf16 mode; the same with and without clipping.  Recorded from the commit before the step
# functions were given one begin and one finish (this test run against that library), not derived here.
COUNTERS = {
    "sgd": (3, 3, 0, 0, 3, 3),
    "train_step": (3, 3, 0, 0, 3, 3),
    "adamw": (3, 0, 3, 0, 0, 3),
    "lamb": (3, 0, 3, 3, 0, 3),
}


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("kind", list(COUNTERS))
def test_step_counters(gpu, kind, clip):
    v = gpu
    m = build(v, "bf16")
    m.set_ema(D)
    m.set_sgd(*SGD)
    if clip:
        m.set_grad_clip(1.0)
    v.kernel_hits_reset()
    for _ in range(3):
        step(m, "sgd" if kind == "train_step" else kind, fused=kind == "train_step")
    hits = v.kernel_hits()
    got = (int(hits[v.HIT_EMA]), int(hits[v.HIT_SGDM]), m.adamw_state()[2] if kind in ("adamw", "lamb") else 0,
           lamb_steps(v, m), m.sgd_info()["steps"], m.ema_info()[1])
    print(f"step counters {kind} clip={clip}: {got}")
    if kind in ("sgd", "train_step"):
        with pytest.raises(v.VitError):
            m.adamw_state()
    m.close()
    assert got == COUNTERS[kind]
