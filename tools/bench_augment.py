"""Cost of RandAugment on the device uint8 batch, HIP events / wall clock.

  ops:   vit_augment_u8 on the context stream, one event pair per call (plan upload + every launch
         of the call), each on a fresh device copy of the batch: every op alone (the same op on all
         images) and a drawn RandAugment(2, 9) plan.  GB/s is over the bytes the op must move, n =
         B * img^2 * 3: 2n for a table lookup or the colour blend (read + write), 3n with image
         statistics (one more read), 4n for sharpness / affine (read + write into the scratch
         buffer, then the copy back).
  steps: vit_trainer_set_batch_u8 (host upload on the copy stream) + vit_trainer_train_step, (a)
         plain and (b) with a drawn plan set before every batch; the two variants alternate in one
         process, wall clock over `--steps` steps after a sync.
    python tools/bench_augment.py [--config vit_b16] [--batch 256] [--iters 20] [--steps 20] [--out FILE]"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vitpkg import vit  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="vit_b16")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    a = vit.augment
    L = vit.lib()
    assert L.vit_init(0) == 0
    cfg = vit.data.CONFIGS[args.config]
    B, img = args.batch, cfg.img
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(3)
    y, x = np.mgrid[0:img, 0:img]
    base = np.stack([np.sin(x / 9.0) * 60 + np.cos(y / 7.0) * 50 + 128] * 3, -1)
    images = np.clip(base[None] + rng.normal(0, 25, (B, img, img, 3)), 0, 255).astype(np.uint8)
    labels = rng.integers(0, cfg.num_classes, B).astype(np.int32)
    n = images.nbytes
    src = vit.DeviceArray.from_numpy(images)
    dev = vit.DeviceArray((B, img, img, 3), np.uint8)
    fill = (ctypes.c_ubyte * 3)(124, 116, 104)
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    cases = [("identity", a.op(a.IDENTITY), 0), ("autocontrast", a.op(a.AUTOCONTRAST), 3),
             ("equalize", a.op(a.EQUALIZE), 3), ("posterize 4", a.op(a.POSTERIZE, iarg=4), 2),
             ("solarize 179", a.op(a.SOLARIZE, iarg=179), 2), ("brightness 1.27", a.op(a.BRIGHTNESS, farg=f32(1.27)), 2),
             ("contrast 1.27", a.op(a.CONTRAST, farg=f32(1.27)), 3), ("color 1.27", a.op(a.COLOR, farg=f32(1.27)), 2),
             ("sharpness 1.27", a.op(a.SHARPNESS, farg=f32(1.27)), 4), ("shear_x 0.09", a.shear_x(0.09), 4),
             ("shear_y 0.09", a.shear_y(0.09), 4), ("translate_x 30", a.translate_x(30.0), 4),
             ("translate_y 30", a.translate_y(30.0), 4), ("rotate 9", a.rotate(9.0, img), 4)]
    plans = [(name, [[o]] * B, mult * n) for name, o, mult in cases]
    drawn = a.RandAugment(2, 9, seed=1).plan(B, img)
    per_op = {o[0]: m for _, o, m in cases}
    drawn_bytes = sum(per_op[o[0]] for row in drawn for o in row) * (n // B)
    # two out-of-place ops in a row need one copy back fewer than two ops alone: an upper figure
    plans.append(("drawn RandAugment(2, 9)", drawn, drawn_bytes))
    say(f"# {args.config} B={B} img={img}: vit_augment_u8, batch of {n / 1e6:.1f} MB, {args.iters} calls each")
    for name, plan, moved in plans:
        arr, batch, depth = a.plan_to_c(plan)
        us = []
        for _ in range(args.iters + 2):
            L.vit_memcpy_d2d(dev.ptr, src.ptr, n)
            L.vit_sync()
            e0, e1 = L.vit_event_create(), L.vit_event_create()
            L.vit_event_record(e0)
            rc = L.vit_augment_u8(dev.ptr, batch, img, arr, depth, fill, None)
            L.vit_event_record(e1)
            L.vit_sync()
            assert rc == 0, vit.check(name)
            us.append(L.vit_event_elapsed_ms(e0, e1) * 1e3)
            L.vit_event_destroy(e0)
            L.vit_event_destroy(e1)
        us = np.array(us[2:])
        med = float(np.median(us))
        rate = f"{moved / 1e6:.1f} MB moved, {moved / med / 1e3:.1f} GB/s" if moved else "nothing moved"
        say(f"{name:24s} median {med:8.1f} us (min {us.min():.1f}, max {us.max():.1f}); {rate}")
    vit.check("augment")

    m = vit.ViT.build(cfg, B, vit.VIT_BF16, params=vit.data.init_params(cfg, "parity", seed=1))

    def steps(with_plan):
        out = []
        for rep in range(args.reps):
            for k in range(args.steps + 3):
                if k == 3:
                    m.sync()
                    t0 = time.perf_counter()
                if with_plan:
                    m.set_augment_plan(drawn, (124, 116, 104))
                m.set_batch_u8(images, labels)
                m.train_step(1e-3)
            m.sync()
            out.append((time.perf_counter() - t0) * 1e3 / args.steps)
        return out

    say(f"# {args.config} B={B} bf16: set_batch_u8 + train_step, ms/step over {args.steps} steps, variants alternating")
    res = {False: [], True: []}
    for rnd in range(3):
        for with_plan in (False, True):
            t = steps(with_plan)
            res[with_plan] += t
            say(f"{'with a drawn (2, 9) plan' if with_plan else 'plain':26s} {' '.join(f'{v:.2f}' for v in t)}")
    p, w = np.array(res[False]), np.array(res[True])
    say(f"plain: median {np.median(p):.2f} ms, spread {p.min():.2f} .. {p.max():.2f}; "
        f"with plan: median {np.median(w):.2f} ms, spread {w.min():.2f} .. {w.max():.2f}")
    slower = np.median(w) - np.median(p)
    say(f"difference of medians {slower:+.3f} ms; spread of the plain runs {p.max() - p.min():.3f} ms -> "
        f"{'within' if slower <= p.max() - p.min() else 'BEYOND'} the plain runs' spread")
    m.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
