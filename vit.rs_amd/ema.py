"""Exponential moving average of the weights (include/vit_trainer.h vit_trainer_set_ema):
timm's ModelEmaV2.  The trainer advances the average on the device inside its optimizer kernels; this
module holds the host side of the recipe: the decay warm-up schedule and the numpy statement of the
update the kernels are checked against bit for bit.  Host-only (numpy): nothing here touches the GPU.
"""
import numpy as np


def one_minus(decay):
    """omd = float32(1.0 - float64(float32(decay))): the library's second coefficient, taken once."""
    return np.float32(1.0 - np.float64(np.float32(decay)))


def ema_ref(e, p, decay):
    """e' = fl32(fl32(d * e) + fl32(omd * p)) in float32, each product and the sum rounded on its own:
    `decay * ema + (1 - decay) * model` as an fp32 framework evaluates it."""
    d, omd = np.float32(decay), one_minus(decay)
    e = np.asarray(e, np.float32)
    p = np.asarray(p, np.float32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        a = (d * e).astype(np.float32)
        b = (omd * p).astype(np.float32)
        return (a + b).astype(np.float32)


def warmup_decay(decay, updates):
    """timm's warm-up: min(decay, (1 + updates) / (10 + updates)) with `updates` the number of optimizer
    steps already averaged (ViT.ema_info()[1]); pass the result to ViT.set_ema before each step."""
    return min(float(decay), (1.0 + updates) / (10.0 + updates))
