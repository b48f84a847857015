"""Cost of momentum SGD in the full step: same-process A/B of ms/step of the fused train step for
  plain     plain SGD (vit_trainer_set_sgd never called, or 0, 0, 0, 0 again),
  momentum  momentum 0.9 (timm's --opt momentum),
  nesterov  momentum 0.9 with Nesterov and weight decay 5e-5 under the no_decay parameter groups
            (timm's --opt sgd; the tiled kernels),
and the optimizer kernel's own time (the trainer's `sgd` timing class: HIP events around the launch) with the
HBM bytes per second it reaches, next to the AdamW kernel's in the same process, each rule in its flat form
(groups off) and its tiled form (all-ones groups).  Bytes per parameter in bf16 / fp8 mode: plain 14 (read p,
g; write p and the bf16 shadow), momentum 22 (+ read and write the buffer), AdamW 30.

The settings are applied between steps and interleaved round by round (cdna_hip_programming.md §5.4 rule 24);
wall clock over `--steps` steps after a sync; the median over the rounds is reported with the spread.
Cases: vit_b16 B=256 bf16 and vit_h14 B=128 fp8 (the early per-chunk update).  Every case runs in a child
process of its own under `timeout`; the first failure ends the run.

    python tools/bench_sgdm.py [--rounds 5 --steps 10] [--out profiles/sgd_momentum_ab.txt]
    python tools/bench_sgdm.py --case vit_b16:256:bf16   # one case, in this process"""
import argparse
import ctypes
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ["vit_b16:256:bf16", "vit_h14:128:fp8"]
MODES = ["plain", "momentum", "nesterov"]
BYTES = {"plain": 14, "momentum": 22, "nesterov": 22, "adamw": 30}
KERNEL_CALLS = 20


def run_case(case, rounds, steps):
    from vitpkg import vit
    model, batch, dtype = case.split(":")
    B = int(batch)
    L = vit.lib()
    assert L.vit_init(0) == 0
    cfg = vit.data.CONFIGS[model]
    m = vit.ViT(cfg, B, vit.VIT_FP8 if dtype == "fp8" else vit.VIT_BF16)
    m.set_params(vit.data.init_params(cfg, "ref", seed=1337))
    px, lab = vit.data.synthetic_batch(cfg, B, seed=1337)
    m.set_batch(px, lab)
    no_decay = vit.groups.no_decay(cfg)

    def apply(mode):
        if mode == "momentum":
            m.set_sgd(**vit.sgd.preset("momentum"))
        elif mode == "nesterov":
            m.set_param_groups(wd_mul=no_decay)
            m.set_sgd(**vit.sgd.preset("sgd", weight_decay=5e-5))

    def leave(mode):
        if mode != "plain":
            m.set_sgd(0, 0, 0, False)
            m.set_param_groups(None, None)

    res = {k: [] for k in MODES}
    for k in MODES:  # warm every mode once
        apply(k)
        m.train_step(1e-4)
        m.sync()
        leave(k)
    for _ in range(rounds):
        for k in MODES:
            apply(k)
            m.train_step(1e-4)
            m.sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                m.train_step(1e-4)
            m.sync()
            res[k].append((time.perf_counter() - t0) / steps * 1e3)
            leave(k)
    vit.check(case)
    base = float(np.median(res["plain"]))
    for k in MODES:
        a = np.array(res[k])
        med = float(np.median(a))
        print(f"RESULT {case:18s} step   {k:10s} median {med:8.3f} ms/step  min {a.min():8.3f}  max {a.max():8.3f}  "
              f"vs plain {100 * (med - base) / base:+6.2f} %  ({rounds} rounds x {steps} steps)", flush=True)
        print(f"rounds {case} {k}: " + " ".join(f"{x:.2f}" for x in a), flush=True)  # (drift over the process)

    # the optimizer kernel alone: the gradients of one backward, then the step call by itself at lr = 0 (the
    # full traffic; the values stay) under the trainer's event timing, the settings interleaved as above
    n = ctypes.c_longlong()
    assert L.vit_layout_query(ctypes.byref(vit._cfg_c(cfg)), None, None, ctypes.byref(n)) > 0
    elems = n.value
    m.zero_grad()
    m.forward_async()
    m.backward()
    m.sync()
    m.set_timing(True)
    ones = np.ones_like(no_decay)
    # (rule, form): flat = groups off; tiled = all-ones groups (the bits of the flat form), nesterov its no_decay table
    kmodes = [(k, f) for k in ("plain", "momentum", "adamw") for f in ("flat", "tiled")] + [("nesterov", "tiled")]
    kres = {km: [] for km in kmodes}
    for r in range(rounds + 1):  # (round 0 warms and is dropped)
        for km in kmodes:
            k, form = km
            apply(k)
            if form == "tiled" and k != "nesterov":
                m.set_param_groups(ones, ones)
            m.timing_reset()
            for _ in range(KERNEL_CALLS):
                if k == "adamw":
                    m.optimizer_step_adamw(0.0, weight_decay=0.05)
                else:
                    m.optimizer_step(0.0)
            m.sync()
            t = m.timing()["sgd"]
            assert t["calls"] == KERNEL_CALLS, t
            if r:
                kres[km].append(t["ms"] / t["calls"])
            m.set_sgd(0, 0, 0, False)
            m.set_param_groups(None, None)
    m.set_timing(False)
    vit.check(case)
    for km in kmodes:
        k, form = km
        a = np.array(kres[km])
        med = float(np.median(a))

        def tbs(ms):
            return BYTES[k] * elems / (ms * 1e-3) / 1e12

        print(f"RESULT {case:18s} kernel {k:9s} {form:5s} median {med * 1e3:8.1f} us  min {a.min() * 1e3:8.1f}  "
              f"max {a.max() * 1e3:8.1f}  {BYTES[k]} B x {elems} elements: {tbs(med):6.3f} TB/s "
              f"(range {tbs(a.max()):.3f} .. {tbs(a.min()):.3f})  ({rounds} rounds x {KERNEL_CALLS} calls)", flush=True)
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--case")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--repeats", type=int, default=1, help="processes per case")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.case:
        run_case(a.case, a.rounds, a.steps)
        return 0
    lines = []
    for case in a.cases.split(","):
        for _ in range(a.repeats):
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--case", case,
                   "--rounds", str(a.rounds), "--steps", str(a.steps)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            print(r.stdout, end="", flush=True)
            if r.returncode != 0:
                print(f"bench_sgdm: case {case} ended with status {r.returncode}; stopping", flush=True)
                return r.returncode
            lines += [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
