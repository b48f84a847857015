"""Cost of random erasing on the device fp32 batch, HIP events / wall clock.

  op:    vit_random_erase_f32 on the context stream, one event pair per call (the list upload and the
         launch), boxes drawn per image with erase.Eraser at prob 0.25 and prob 1 (timm's area and aspect
         defaults, one box), each mode; `--iters` calls per case, the whole table measured twice and the
         second run reported.  GB/s is over the bytes written, 12 bytes per covered pixel.
  steps: vit_trainer_set_batch_u8 + vit_trainer_train_step, (a) plain and (b) with a drawn (0.25, PIXEL, 1)
         erase (host draw + vit_trainer_erase_batch) between the two; the variants alternate in one
         process, wall clock over `--steps` steps after a sync.
    python tools/bench_erase.py [--config vit_b16] [--batch 256] [--iters 20] [--steps 20] [--out FILE]"""
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
    ap.add_argument("--no-steps", action="store_true", help="the op table only")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    er = vit.erase
    L = vit.lib()
    assert L.vit_init(0) == 0
    cfg = vit.data.CONFIGS[args.config]
    B, img = args.batch, cfg.img
    P = ctypes.c_void_p
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(3)
    dev = vit.DeviceArray.from_numpy(rng.standard_normal((B, 3, img, img)).astype(np.float32))
    keys = np.arange(B, dtype=np.int64)
    seed = 1337
    names = {er.ERASE_CONST: "const", er.ERASE_RAND: "rand", er.ERASE_PIXEL: "pixel"}
    say(f"# {args.config} B={B} img={img}: vit_random_erase_f32, batch of {dev.nbytes / 1e6:.1f} MB, "
        f"{args.iters} calls each, second of two runs")
    for run in range(2):
        for prob in (0.25, 1.0):
            boxes = er.Eraser(prob=prob, seed=seed).boxes(keys, img)
            covered = int(((boxes[:, 0, 2] - boxes[:, 0, 0]) * (boxes[:, 0, 3] - boxes[:, 0, 1])).sum())
            written = covered * 12
            for mode in (er.ERASE_CONST, er.ERASE_RAND, er.ERASE_PIXEL):
                us = []
                for _ in range(args.iters + 2):
                    L.vit_sync()
                    e0, e1 = L.vit_event_create(), L.vit_event_create()
                    L.vit_event_record(e0)
                    rc = L.vit_random_erase_f32(dev.ptr, B, img, boxes.ctypes.data_as(P), 1, mode,
                                                ctypes.c_ulonglong(seed), keys.ctypes.data_as(P), None)
                    L.vit_event_record(e1)
                    L.vit_sync()
                    assert rc == 0, vit.check(names[mode])
                    us.append(L.vit_event_elapsed_ms(e0, e1) * 1e3)
                    L.vit_event_destroy(e0)
                    L.vit_event_destroy(e1)
                us = np.array(us[2:])
                med = float(np.median(us))
                if run == 1:
                    say(f"prob {prob:4.2f} {names[mode]:6s} {int((boxes[:, 0, 2] > boxes[:, 0, 0]).sum()):4d} boxes "
                        f"median {med:8.1f} us (min {us.min():.1f}, max {us.max():.1f}); "
                        f"{written / 1e6:.1f} MB written, {written / med / 1e3:.1f} GB/s")
    vit.check("random_erase")
    dev.free()
    if args.no_steps:
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return

    y, x = np.mgrid[0:img, 0:img]
    base = np.stack([np.sin(x / 9.0) * 60 + np.cos(y / 7.0) * 50 + 128] * 3, -1)
    images = np.clip(base[None] + rng.normal(0, 25, (B, img, img, 3)), 0, 255).astype(np.uint8)
    labels = rng.integers(0, cfg.num_classes, B).astype(np.int32)
    m = vit.ViT.build(cfg, B, vit.VIT_BF16, params=vit.data.init_params(cfg, "parity", seed=1))
    eraser = er.Eraser(prob=0.25, mode=er.ERASE_PIXEL, seed=seed)
    step_no = [0]

    def steps(with_erase):
        out = []
        for rep in range(args.reps):
            for k in range(args.steps + 3):
                if k == 3:
                    m.sync()
                    t0 = time.perf_counter()
                m.set_batch_u8(images, labels)
                if with_erase:
                    eraser.apply(m, er.Eraser.keys_for_step(step_no[0], B))
                    step_no[0] += 1
                m.train_step(1e-3)
            m.sync()
            out.append((time.perf_counter() - t0) * 1e3 / args.steps)
        return out

    say(f"# {args.config} B={B} bf16: set_batch_u8 + train_step, ms/step over {args.steps} steps, variants alternating")
    res = {False: [], True: []}
    for rnd in range(3):
        for with_erase in (False, True):
            t = steps(with_erase)
            res[with_erase] += t
            say(f"{'with a drawn (0.25, pixel, 1) erase' if with_erase else 'plain':36s} {' '.join(f'{v:.2f}' for v in t)}")
    p, w = np.array(res[False]), np.array(res[True])
    say(f"plain: median {np.median(p):.2f} ms, spread {p.min():.2f} .. {p.max():.2f}; "
        f"with erase: median {np.median(w):.2f} ms, spread {w.min():.2f} .. {w.max():.2f}")
    slower = np.median(w) - np.median(p)
    say(f"difference of medians {slower:+.3f} ms; spread of the plain runs {p.max() - p.min():.3f} ms -> "
        f"{'within' if slower <= p.max() - p.min() else 'BEYOND'} the plain runs' spread")
    m.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
