"""LAMB reference (include/vit_trainer.h vit_trainer_step_lamb) in numpy: every operation
rounded to the working precision on its own (fp32 by default), the two sums of squares in float64, and the
bias corrections as the oracle's ref_adamw_step rounds them (pow in double, then the working precision).
One call is one segment: a (tensor, layer) slice of the canonical arrays.

The GPU tests compare in stages (tests/test_gpu_gradclip.py's rules): m, v bit-exact; the norms within one
fp32 ulp of norms(); the ratio bit-exact from the device's own norms (ratio()); p' bit-exact from the
device's own ratio (apply())."""
import numpy as np

F32 = np.float32
ALWAYS_ADAPT, TRUST_CLIP = 1, 2


def bias_corrections(beta1, beta2, t, dt=F32):
    """1 - beta^t: the power in double of the beta as the working precision holds it"""
    return dt(1) - dt(float(dt(beta1)) ** t), dt(1) - dt(float(dt(beta2)) ** t)


def clip_g(g, c, dt=F32):
    """g' = c * g rounded on its own (c None: no clipping)"""
    return g if c is None else (dt(c) * g).astype(dt)


def moments(p, g, m, v, beta1, beta2, eps, wd_e, t, dt=F32):
    """(m', v', u): adamw_update's two lines, then the bracket of its last one"""
    b1, b2 = dt(beta1), dt(beta2)
    omb1, omb2 = dt(1) - b1, dt(1) - b2
    bc1, bc2 = bias_corrections(beta1, beta2, t, dt)
    with np.errstate(all="ignore"):
        mi = (b1 * m + omb1 * g).astype(dt)
        vi = (b2 * v + omb2 * g * g).astype(dt)
        mh, vh = (mi / bc1).astype(dt), (vi / bc2).astype(dt)
        u = (mh / (np.sqrt(vh) + dt(eps)) + dt(wd_e) * p).astype(dt)
    assert mi.dtype == dt and vi.dtype == dt and u.dtype == dt
    return mi, vi, u


def norms(p, u, dt=F32):
    """(wn, un): the square roots of the float64 sums of squares, rounded to the working precision"""
    W = np.sum(np.square(p.astype(np.float64)))
    U = np.sum(np.square(u.astype(np.float64)))
    return dt(np.sqrt(W)), dt(np.sqrt(U))


def ratio(wn, un, wd_e, flags, dt=F32):
    wn, un = dt(wn), dt(un)
    adapt = bool(flags & ALWAYS_ADAPT) or dt(wd_e) != 0
    r = wn / un if (adapt and wn > 0 and un > 0) else dt(1)
    if (flags & TRUST_CLIP) and not r < dt(1):
        r = dt(1)
    return dt(r)


def apply(p, u, lr_e, r, dt=F32):
    """p' = p - (lr_e * r) * u"""
    step = dt(dt(lr_e) * dt(r))
    with np.errstate(all="ignore"):
        return (p - (step * u).astype(dt)).astype(dt)


def lamb_segment(p, g, m, v, lr_e, beta1, beta2, eps, wd_e, t, flags=0, c=None, r=None, dt=F32):
    """One LAMB step of one segment -> dict(p, m, v, u, wn, un, r).  r given: the ratio to apply (the
    device's own, or 1 for the AdamW comparison) in place of the one computed here."""
    p, g, m, v = (np.ascontiguousarray(a, dtype=dt) for a in (p, g, m, v))
    mi, vi, u = moments(p, clip_g(g, c, dt), m, v, beta1, beta2, eps, wd_e, t, dt)
    wn, un = norms(p, u, dt)
    r_own = ratio(wn, un, wd_e, flags, dt)
    return {"p": apply(p, u, lr_e, r_own if r is None else r, dt), "m": mi, "v": vi, "u": u, "wn": wn, "un": un,
            "r": r_own}


def group_hp(base, mul, dt=F32):
    """lr_e / wd_e: one multiply rounded on its own"""
    return dt(dt(base) * dt(mul))


def ulp_apart(a, b):
    """distance in fp32 ulps between two positive finite fp32 values (or 0 for equal bits)"""
    return abs(int(F32(a).view(np.uint32)) - int(F32(b).view(np.uint32)))
