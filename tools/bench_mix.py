"""Cost of the batch-mix kernels and of a soft-target step, HIP events / wall clock.

  kernels: vit_trainer_mix_batch alone on the trainer's stream, one event pair per launch, each on
           a batch freshly copied on the device (a batch can be mixed once).  Mixup reads and writes
           every pixel of every pair: 2 * B * 3 * img^2 * 4 bytes.
  steps:   vit_trainer_train_step after a device-side set_batch, (a) plain and (b) with label
           smoothing 0.1 and a mixup of every batch; wall clock over `--steps` steps after a sync.
    python tools/bench_mix.py [--config vit_b16] [--batch 256] [--iters 20] [--steps 20]"""
import argparse
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
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp8"])
    a = ap.parse_args()
    L = vit.lib()
    assert L.vit_init(0) == 0
    cfg = vit.data.CONFIGS[a.config]
    B, img = a.batch, cfg.img
    px, lab = vit.data.synthetic_batch(cfg, B, seed=2)
    dpx = vit.DeviceArray.from_numpy(px)
    dlab = vit.DeviceArray.from_numpy(lab, np.int32)
    m = vit.ViT.build(cfg, B, vit.VIT_BF16 if a.precision == "bf16" else vit.VIT_FP8,
                      params=vit.data.init_params(cfg, "parity", seed=1))
    L.vit_set_stream(L.vit_trainer_stream(m.h))  # vit_event_record follows the trainer's stream

    def fresh():
        assert L.vit_trainer_set_batch_device(m.h, dpx.ptr, dlab.ptr) == 0

    nbytes = 2 * B * 3 * img * img * 4
    side = int(img * np.sqrt(0.5))
    cases = [("mixup lam 0.3", nbytes, (vit.MIX_MIXUP, 0.3, None)),
             ("cutmix half-area box", 2 * (B // 2 * 2) * 3 * side * side * 4,
              (vit.MIX_CUTMIX, 1.0, (20, 20, 20 + side, 20 + side)))]
    for name, moved, mix in cases:
        us = []
        for _ in range(a.iters + 2):
            fresh()
            e0, e1 = L.vit_event_create(), L.vit_event_create()
            L.vit_event_record(e0)
            m.mix_batch(*mix)
            L.vit_event_record(e1)
            m.sync()
            us.append(L.vit_event_elapsed_ms(e0, e1) * 1e3)
            L.vit_event_destroy(e0)
            L.vit_event_destroy(e1)
        us = np.array(us[2:])
        med = float(np.median(us))
        print(f"{a.config} B={B} {name}: median {med:.1f} us (min {us.min():.1f}, max {us.max():.1f}; "
              f"{a.iters} launches), {moved / 1e6:.1f} MB moved, {moved / med / 1e6:.2f} TB/s", flush=True)
    vit.check("mix")

    def steps(soft):
        m.set_label_smoothing(0.1 if soft else 0.0)
        out = []
        for rep in range(3):
            for k in range(a.steps + 3):
                if k == 3:
                    m.sync()
                    t0 = time.perf_counter()
                fresh()
                if soft:
                    m.mix_batch(vit.MIX_MIXUP, 0.3)
                m.train_step(1e-3)
            m.sync()
            out.append((time.perf_counter() - t0) * 1e3 / a.steps)
        return out

    for rep in range(2):  # interleaved: plain, soft, plain, soft
        for soft in (False, True):
            t = steps(soft)
            print(f"{a.config} B={B} {a.precision} set_batch_device + train_step, "
                  f"{'smoothing 0.1 + mixup' if soft else 'plain'}: "
                  f"{' '.join(f'{x:.2f}' for x in t)} ms/step ({B / min(t) * 1e3:.0f} img/s best)", flush=True)
    L.vit_set_stream(None)
    m.close()


if __name__ == "__main__":
    main()
