"""Gradient accumulation over micro-batches (include/vit_trainer.h vit_trainer_set_grad_accum).
The trainer sums the gradients of a window's backwards on the device; this module holds the host side: the
number of micro-steps a global batch needs and the numpy statement of the sum the device is checked against
bit for bit.  Host-only (numpy): nothing here touches the GPU.
"""
import numpy as np


def accum_ref(grads):
    """(((g1 + g2) + g3) + ... + gN) in float32, left to right, each sum rounded to fp32 once: the window's
    statement.  `grads` is a non-empty sequence of equally shaped arrays."""
    grads = list(grads)
    if not grads:
        raise ValueError("accum_ref: no gradients")
    acc = np.array(grads[0], dtype=np.float32, copy=True)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for g in grads[1:]:
            acc = (acc + np.asarray(g, np.float32)).astype(np.float32)
    return acc


def plan(global_batch, batch, world=1):
    """steps for ViT.set_grad_accum so that steps * batch * world == global_batch (the b_global to pass on
    several ranks).  Raises ValueError unless global_batch is a positive multiple of batch * world."""
    for name, v in (("global_batch", global_batch), ("batch", batch), ("world", world)):
        if int(v) != v or int(v) < 1:
            raise ValueError(f"accum.plan: {name} {v!r} is not a positive integer")
    per_step = int(batch) * int(world)
    if int(global_batch) % per_step:
        raise ValueError(f"accum.plan: global batch {global_batch} is not a multiple of batch {batch} x world "
                         f"{world} = {per_step}")
    return int(global_batch) // per_step
