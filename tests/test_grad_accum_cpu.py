"""Gradient accumulation, host side (vit.rs_amd/accum.py, include/vit_trainer.h vit_trainer_set_grad_accum,
DESIGN.md §20): the numpy statement of a window's sum, the plan of micro-steps for a global batch, and the
new names of the library.  No GPU."""
import os

import numpy as np
import pytest

F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------ accum_ref
def test_accum_ref_keeps_the_stated_order(vit):
    """(a + b) + c, each sum rounded to fp32 once: 1 is lost against 2^24 when it is added alone, and the two
    ones together are not"""
    a, b, c = F32(2.0 ** 24), F32(1.0), F32(1.0)
    left = F32(F32(a + b) + c)
    right = F32(a + F32(b + c))
    assert left == F32(2.0 ** 24) and right == F32(2.0 ** 24 + 2.0) and left != right
    got = vit.accum.accum_ref([np.array([a, b], F32), np.array([b, a], F32), np.array([c, c], F32)])
    assert got.dtype == np.float32
    assert np.array_equal(bits(got), bits(np.array([left, left], F32)))
    # the other association, spelled through the same function, is the other value
    other = vit.accum.accum_ref([np.array([a], F32), vit.accum.accum_ref([np.array([b], F32), np.array([c], F32)])])
    assert other[0] == right


def test_accum_ref_is_the_stepwise_rounded_float64_sum(vit):
    rng = np.random.default_rng(5)
    gs = [(rng.standard_normal(4099) * 10.0 ** rng.integers(-3, 4, 4099)).astype(F32) for _ in range(4)]
    gs[1][:4] = [0.0, -0.0, 1e-45, 3e38]
    gs[2][:4] = [-0.0, -0.0, -3e-42, 3e38]  # (-0) + (-0) = -0; a denormal sum; an overflow to +inf
    want = gs[0].astype(np.float64)
    with np.errstate(over="ignore"):
        for g in gs[1:]:
            want = (want + g.astype(np.float64)).astype(F32).astype(np.float64)  # 53 >= 2 * 24 + 2: one rounding
    got = vit.accum.accum_ref(gs)
    assert np.array_equal(bits(got), bits(want.astype(F32)))
    assert np.isinf(got[3]) and np.signbit(got[1])
    # one term: a copy, not a view
    one = vit.accum.accum_ref([gs[0]])
    assert np.array_equal(bits(one), bits(gs[0])) and one is not gs[0]
    one[0] = 7
    assert gs[0][0] != 7
    with pytest.raises(ValueError):
        vit.accum.accum_ref([])


# ------------------------------------------------------------------ plan
def test_plan_values(vit):
    plan = vit.accum.plan
    assert plan(1024, 256) == 4
    assert plan(4096, 128, world=8) == 4
    assert plan(256, 256) == 1
    assert plan(2048, 256, 8) == 1
    assert plan(6, 3) == 2
    assert isinstance(plan(np.int64(1024), np.int32(256)), int)


@pytest.mark.parametrize("args", [(1000, 256), (256, 256, 2), (0, 256), (-256, 256), (1024, 0), (1024, 256, 0),
                                  (1024, -256), (1024.5, 256), (100, 256)])
def test_plan_errors(vit, args):
    with pytest.raises(ValueError):
        vit.accum.plan(*args)


# ------------------------------------------------------------------ the library's names
def test_symbols_and_wrappers(vit):
    names = vit.exported_symbols()
    for s in ("vit_trainer_set_grad_accum", "vit_trainer_get_grad_accum_info", "vit_trainer_get_grad_accum",
              "grad_accumulate"):
        assert s in names, s
        assert hasattr(vit.lib(), s), s
    for meth in ("set_grad_accum", "grad_accum_info", "grad_accum"):
        assert callable(getattr(vit.ViT, meth)), meth
    assert callable(vit.grad_accumulate)
    assert vit.HIT_ACCUM == 98 < len(vit.kernel_hits())
    # the declarations are in the public headers
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(vit.__file__))), "include")
    text = "".join(open(os.path.join(inc, f)).read() for f in ("vit_trainer.h", "vit_ops.h"))
    for s in names:
        if "accum" in s:
            assert s + "(" in text, s
    assert "VIT_HIT_ACCUM = 98" in text and "VIT_HIT_COUNT = 99" in text
