"""The checkpoint format as include/vit_checkpoint.h documents it, stated in numpy and independent of
vit.rs_amd/csrc/checkpoint.cpp: the 256-int little-endian header, slots [0..26], then the fp32 sections in file
order (params, m, v, ema, momentum).  encode() takes vit.write_checkpoint's arguments and returns the file's
bytes.  Shared by tests/test_checkpoint_sections_cpu.py and tests/test_gpu_checkpoint_paths.py."""
import itertools

import numpy as np

MAGIC, VERSION, HEADER_BYTES = 20261016, 1, 1024
# (AdamW state, EMA, momentum buffer): all eight layouts
LAYOUTS = list(itertools.product((False, True), repeat=3))


def f32_bits(x):
    return int(np.array([x], "<f4").view("<u4")[0])


def lo_hi(x):
    return x & 0xFFFFFFFF, (x >> 32) & 0xFFFFFFFF


def header(cfg, has_opt, step=0, adamw=None, has_ema=False, ema_decay=0.0, ema_updates=0, has_momentum=False,
           sgd=None, momentum_steps=0):
    h = np.zeros(HEADER_BYTES // 4, "<u4")
    n = cfg.num_params()
    h[0], h[1] = MAGIC, VERSION
    h[2] = (cfg.img // cfg.patch) ** 2 + 1
    h[3], h[4], h[5], h[6] = cfg.num_classes, cfg.num_layers, cfg.num_heads, cfg.channels
    h[7], h[8], h[9] = cfg.img, cfg.patch, cfg.in_ch
    h[10] = (1 if has_opt else 0) | (2 if has_ema else 0) | (4 if has_momentum else 0)
    h[12], h[13] = lo_hi(n)
    if has_opt:
        h[11] = step
        if adamw is not None:
            h[14:18] = [f32_bits(x) for x in adamw]
    if has_ema:
        h[18] = f32_bits(ema_decay)
        h[19], h[20] = lo_hi(ema_updates)
    if has_momentum:
        h[21], h[22] = lo_hi(momentum_steps)
        h[23:26] = [f32_bits(x) for x in sgd[:3]]
        h[26] = 1 if sgd[3] else 0
    return h


def encode(cfg, params, m=None, v=None, step=0, adamw=None, ema=None, ema_decay=0.0, ema_updates=0, momentum=None,
           sgd=None, momentum_steps=0):
    assert (m is None) == (v is None)
    h = header(cfg, m is not None, step, adamw, ema is not None, ema_decay, ema_updates, momentum is not None, sgd,
               momentum_steps)
    out = [h.tobytes()]
    for a in (params, m, v, ema, momentum):
        if a is not None:
            a = np.ascontiguousarray(a, "<f4")
            assert a.size == cfg.num_params()
            out.append(a.tobytes())
    return b"".join(out)
