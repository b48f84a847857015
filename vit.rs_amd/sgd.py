"""Momentum SGD (include/vit_trainer.h vit_trainer_set_sgd): torch.optim.SGD's update with
momentum, dampening, Nesterov and coupled weight decay.  The trainer runs it inside its optimizer kernels;
this module holds the host side: timm's two presets and the numpy statement of the update the kernels are
checked against bit for bit.  Host-only (numpy): nothing here touches the GPU.
"""
import numpy as np

# timm's --opt names: `momentum` is SGD with momentum 0.9, `sgd` the same with Nesterov.  Keyword arguments
# of ViT.set_sgd; the weight decay is the recipe's own.
PRESETS = {
    "momentum": dict(momentum=0.9, dampening=0.0, nesterov=False),
    "sgd": dict(momentum=0.9, dampening=0.0, nesterov=True),
}


def preset(name, weight_decay=0.0):
    """Keyword arguments of ViT.set_sgd for timm's `--opt momentum` / `--opt sgd`."""
    if name not in PRESETS:
        raise ValueError(f"unknown preset {name!r} (one of {sorted(PRESETS)})")
    return dict(PRESETS[name], weight_decay=float(weight_decay))


def one_minus(dampening, dtype=np.float32):
    """omd = dtype(1.0 - float64(dtype(dampening))): the library's second coefficient, taken once."""
    return dtype(1.0 - np.float64(dtype(dampening)))


def sgd_ref(p, g, buf, first, lr, momentum, dampening, weight_decay, nesterov, c=None, dtype=np.float32):
    """One step on arrays of one parameter group, every operation rounded to `dtype` on its own:

        g1 = c * g                      (c None: g)
        g2 = g1 + wd * p                (wd == 0: g1; torch skips the term, so does the library)
        b' = g2                         (first: torch's buf = grad.clone(), signed zeros included)
           = mu * b + omd * g2          (otherwise)
        d  = g2 + mu * b'               (nesterov; otherwise b')
        p' = p - lr * d

    lr and weight_decay are the group's own values (lr_e, wd_e).  Returns (p', b'); buf may be None when first.
    dtype=np.float64 is the form compared with torch.optim.SGD in float64."""
    t = dtype
    p = np.asarray(p, t)
    g = np.asarray(g, t)
    lr, mu, wd, omd = t(lr), t(momentum), t(weight_decay), one_minus(dampening, t)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        g1 = g if c is None else (t(c) * g).astype(t)
        g2 = (g1 + (wd * p).astype(t)).astype(t) if wd != 0 else g1
        if first:
            b = g2.copy()
        else:
            b = ((mu * np.asarray(buf, t)).astype(t) + (omd * g2).astype(t)).astype(t)
        d = (g2 + (mu * b).astype(t)).astype(t) if nesterov else b
        return (p - (lr * d).astype(t)).astype(t), b
