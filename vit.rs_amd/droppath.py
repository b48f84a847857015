"""Stochastic depth (drop path): the per-step table of residual-branch scales.

draw() wraps the library's host-only vit_drop_path_draw; reference_draw() is its Python statement;
DropPath draws a table per step and hands it to ViT.set_drop_path.  Host-only: nothing here
touches the GPU.
"""
import ctypes

import numpy as np

DRAW_TAG = 0x64726F7070617468  # "droppath"
_M = (1 << 64) - 1


def splitmix64(seed, i):
    z = (seed + (i + 1) * 0x9E3779B97F4A7C15) & _M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M
    return z ^ (z >> 31)


def rates(L, rate, linear=True):
    """p_l per layer as float32: timm's linspace(0, rate, L) when linear (rate itself for L == 1)."""
    r = np.float32(rate)
    if not linear or L == 1:
        return np.full(L, r, np.float32)
    return np.array([np.float32(float(r) * l / (L - 1)) for l in range(L)], np.float32)


def reference_draw(seed, key, L, B, rate, linear=True):
    """The table [L, 2, B] float32 as vit_drop_path_draw computes it, bit for bit."""
    assert L >= 1 and B >= 1 and 0.0 <= float(np.float32(rate)) < 1.0
    s = (seed & _M) ^ splitmix64(DRAW_TAG, key & _M)
    p = rates(L, rate, linear)
    out = np.zeros((L, 2, B), np.float32)
    for l in range(L):
        keep = np.float32(1.0) / (np.float32(1.0) - p[l])
        for br in range(2):
            for b in range(B):
                u = np.float32(splitmix64(s, (2 * l + br) * B + b) >> 40) * np.float32(2.0 ** -24)
                out[l, br, b] = keep if u >= p[l] else np.float32(0.0)
    return out


def draw(seed, key, L, B, rate, linear=True):
    """vit_drop_path_draw: the table [L, 2, B] float32 of scales 0 or 1 / (1 - p_l)."""
    from . import check, lib
    out = np.empty((L, 2, B), np.float32)
    if lib().vit_drop_path_draw(ctypes.c_ulonglong(seed & _M), int(key), int(L), int(B), float(rate), int(linear),
                                out.ctypes.data_as(ctypes.c_void_p)):
        check("vit_drop_path_draw")
        raise ValueError("vit_drop_path_draw failed")
    return out


class DropPath:
    """Stochastic depth at `rate` (the last layer's when linear, timm's drop_path_rate).

    apply(model, step, rank=0, world=1) draws the table of key step * world + rank (ranks of a
    data-parallel job draw different masks) and sets it for the model's next training forward;
    rate 0 sets nothing.  Returns the table (None at rate 0)."""

    def __init__(self, rate=0.1, linear=True, seed=1337):
        assert 0.0 <= rate < 1.0
        self.rate, self.linear, self.seed = float(rate), bool(linear), int(seed)

    def apply(self, model, step, rank=0, world=1):
        if self.rate == 0.0:
            return None
        tab = draw(self.seed, int(step) * int(world) + int(rank), model.cfg.num_layers, model.B, self.rate,
                   self.linear)
        model.set_drop_path(tab)
        return tab
