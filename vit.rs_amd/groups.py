"""Parameter groups: per-tensor, per-layer multipliers of the learning rate and of the weight decay
(include/vit_trainer.h vit_trainer_set_param_groups) and the two tables every ViT
recipe builds from them.

A table is a float32 array [20, L]: row ti is tensor ti of the canonical order (data.PARAM_NAMES),
column l the layer; the tensors outside the blocks (patch_w .. wpe, lnfw .. head_b) use column 0 and
their other columns are ignored.  Host-only (numpy): nothing here touches the GPU.
"""
import numpy as np

from .data import LAYER_PARAMS, PARAM_NAMES

# tensors a weight-decay exclusion list names: every 1-D tensor (biases, LayerNorm gains and biases),
# the class token and the position embedding
_MATRICES = ("patch_w", "qkvw", "attprojw", "fcw", "fcprojw", "head_w")


def expand(cfg, table):
    """A multiplier table as float32 [20, L] from None (ones), an array of that shape, or a dict
    {tensor name: scalar or length-L sequence}; names a dict leaves out get 1.  A per-layer sequence
    for a tensor outside the blocks, an unknown name or a wrong length raises ValueError."""
    L = cfg.num_layers
    out = np.ones((len(PARAM_NAMES), L), np.float32)
    if table is None:
        return out
    if isinstance(table, dict):
        for name, val in table.items():
            if name not in PARAM_NAMES:
                raise ValueError(f"unknown tensor name {name!r} (one of {PARAM_NAMES})")
            a = np.asarray(val, np.float32)
            if a.ndim == 0:
                out[PARAM_NAMES.index(name), :] = a
            elif a.ndim == 1 and name in LAYER_PARAMS and a.size == L:
                out[PARAM_NAMES.index(name), :] = a
            else:
                want = f"a scalar or {L} values" if name in LAYER_PARAMS else "a scalar"
                raise ValueError(f"{name}: expected {want}, got shape {a.shape}")
        return out
    a = np.asarray(table, np.float32)
    if a.shape != out.shape:
        raise ValueError(f"expected an array of shape {out.shape}, got {a.shape}")
    return np.ascontiguousarray(a)


def no_decay(cfg):
    """wd_mul that keeps weight decay off everything but the weight matrices: 0 for every 1-D tensor
    (all biases, all LayerNorm gains and biases), cls and wpe; 1 for patch_w, the four block weights
    and head_w (the exclusion list of timm / DeiT / MAE / BEiT)."""
    out = np.zeros((len(PARAM_NAMES), cfg.num_layers), np.float32)
    for name in _MATRICES:
        out[PARAM_NAMES.index(name), :] = 1.0
    return out


def layer_ids(cfg):
    """The BEiT / MAE layer id of every table entry, int [20, L]: patch_w, patch_b, cls, wpe 0;
    block l is l + 1; lnfw, lnfb, head_w, head_b L + 1."""
    L = cfg.num_layers
    ids = np.zeros((len(PARAM_NAMES), L), np.int64)
    for ti, name in enumerate(PARAM_NAMES):
        if name in LAYER_PARAMS:
            ids[ti, :] = np.arange(L) + 1
        elif name in ("lnfw", "lnfb", "head_w", "head_b"):
            ids[ti, :] = L + 1
    return ids


def layer_decay(cfg, decay):
    """lr_mul of layer-wise learning-rate decay: decay ** (L + 1 - id) with the ids of layer_ids(),
    computed in double and rounded to float32 (the head trains at lr, the embedding at
    lr * decay ** (L + 1))."""
    ids = layer_ids(cfg)
    return (np.float64(decay) ** (cfg.num_layers + 1 - ids).astype(np.float64)).astype(np.float32)
