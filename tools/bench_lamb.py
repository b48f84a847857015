"""Cost of LAMB against AdamW in the full step: same-process A/B of ms/step for
  adamw / lamb            forward + backward + the optimizer step,
  adamw_ema / lamb_ema    the same with the EMA of the weights on (fused into the optimizer kernels),
  adamw_clip / lamb_clip  the same with global-norm clipping on (max_norm = inf: computed, never scaling),
and of the optimizer step alone (`opt` rows: `--steps` optimizer calls back to back on the gradients as they
stand, no forward or backward between them), with the HBM bandwidth that time means at AdamW's 30 B and LAMB's
42 B per parameter (the bf16 shadow's 2 B included; + 8 B with the EMA, + 4 B for the clip's norm pass).

The modes are applied between steps and interleaved round by round (cdna_hip_programming.md §5.4 rule 24);
wall clock over `--steps` steps after a sync; the median over the rounds is reported with the spread.  Cases:
vit_b16 B=256 bf16 and vit_h14 B=128 fp8.  Every case runs in a child process of its own under `timeout`; the
first failure ends the run.

    python tools/bench_lamb.py [--rounds 5 --steps 10] [--out profiles/lamb_ab.txt]
    python tools/bench_lamb.py --case vit_b16:256:bf16   # one case, in this process"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ["vit_b16:256:bf16", "vit_h14:128:fp8"]
MODES = ["adamw", "lamb", "adamw_ema", "lamb_ema", "adamw_clip", "lamb_clip"]
DECAY = 0.9999
BYTES = {"adamw": 30, "lamb": 42}  # per parameter with the bf16 shadow; + 8 with the EMA


def run_case(case, rounds, steps, only=None):
    from vitpkg import vit
    model, batch, dtype = case.split(":")
    B = int(batch)
    assert vit.lib().vit_init(0) == 0
    modes = [k for k in MODES if not only or k in only]
    cfg = vit.data.CONFIGS[model]
    m = vit.ViT(cfg, B, vit.VIT_FP8 if dtype == "fp8" else vit.VIT_BF16)
    m.set_params(vit.data.init_params(cfg, "ref", seed=1337))
    px, lab = vit.data.synthetic_batch(cfg, B, seed=1337)
    m.set_batch(px, lab)
    nparam = cfg.num_params()

    def apply(mode):
        if mode.endswith("_ema"):
            m.set_ema(DECAY)
        if mode.endswith("_clip"):
            m.set_grad_clip(float("inf"))

    def leave(mode):
        if mode.endswith("_ema"):
            m.set_ema(0)
        if mode.endswith("_clip"):
            m.set_grad_clip(0.0)

    def opt(mode):
        if mode.startswith("lamb"):
            m.optimizer_step_lamb(1e-4, weight_decay=0.05)
        else:
            m.optimizer_step_adamw(1e-4, weight_decay=0.05)

    def step(mode):
        m.zero_grad()
        m.forward_async()
        m.backward()
        opt(mode)

    full, alone = {k: [] for k in modes}, {k: [] for k in modes}
    for k in modes:  # warm every mode once
        apply(k)
        step(k)
        m.sync()
        leave(k)
    for _ in range(rounds):
        for k in modes:
            apply(k)
            step(k)
            m.sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                step(k)
            m.sync()
            full[k].append((time.perf_counter() - t0) / steps * 1e3)
            t0 = time.perf_counter()
            for _ in range(steps):
                opt(k)
            m.sync()
            alone[k].append((time.perf_counter() - t0) / steps * 1e3)
            leave(k)
    vit.check(case)
    base = {k: float(np.median(full[k.replace("lamb", "adamw")])) for k in modes if k.replace("lamb", "adamw") in full}
    for k in modes:
        a, o = np.array(full[k]), np.array(alone[k])
        med, omed = float(np.median(a)), float(np.median(o))
        by = BYTES[k.split("_")[0]] + (8 if k.endswith("_ema") else 0) + (4 if k.endswith("_clip") else 0)
        d = f"vs {k.replace('lamb', 'adamw'):10s} {med - base[k]:+7.3f} ms" if k in base else ""
        print(f"RESULT {case:18s} {k:11s} median {med:8.3f} ms/step  min {a.min():8.3f}  max {a.max():8.3f}  {d}  | "
              f"opt alone {omed:7.3f} ms  min {o.min():7.3f}  max {o.max():7.3f}  = {by * nparam / omed / 1e9:6.2f} TB/s "
              f"at {by} B/param  ({rounds} rounds x {steps} steps)", flush=True)
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--case")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--modes", help="comma list: only these modes")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.case:
        run_case(a.case, a.rounds, a.steps, a.modes.split(",") if a.modes else None)
        return 0
    lines = []
    for case in a.cases.split(","):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--case", case,
               "--rounds", str(a.rounds), "--steps", str(a.steps)] + (["--modes", a.modes] if a.modes else [])
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        print(r.stdout, end="", flush=True)
        if r.returncode != 0:
            print(f"bench_lamb: case {case} ended with status {r.returncode}; stopping", flush=True)
            return r.returncode
        lines += [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
