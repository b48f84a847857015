"""Cost of the EMA of the weights in the full step: same-process A/B of ms/step for
  off       EMA never on (the optimizer kernels as they are without it),
  fused     EMA on, the update inside the optimizer kernels (8 B per parameter more HBM traffic),
  separate  EMA on with option ema_fused = 0: ema_update launched behind each optimizer kernel (12 B).

The modes are applied between steps and interleaved round by round (cdna_hip_programming.md §5.4
rule 24); wall clock over `--steps` steps after a sync; the median over the rounds is reported with
the spread.  Cases: vit_b16 B=256 bf16 with SGD (the fused train step) and with AdamW, vit_h14 B=128
fp8 with SGD (the early per-chunk SGD).  Every case runs in a child process of its own under
`timeout`, twice; the first failure ends the run.

    python tools/bench_ema.py [--rounds 5 --steps 10] [--out profiles/ema_ab.txt]
    python tools/bench_ema.py --other-lib PATH    # + the `off` step of another build of the library
                                                  #   (e.g. the parent commit's) between the two
    python tools/bench_ema.py --case vit_b16:256:bf16:sgd   # one case, in this process"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ["vit_b16:256:bf16:sgd", "vit_b16:256:bf16:adamw", "vit_h14:128:fp8:sgd"]
MODES = ["off", "fused", "separate"]
DECAY = 0.9999


def run_case(case, rounds, steps, only=None):
    from vitpkg import vit
    model, batch, dtype, opt = case.split(":")
    B = int(batch)
    L = vit.lib()
    assert L.vit_init(0) == 0
    has_ema = hasattr(L, "vit_trainer_set_ema")
    modes = MODES if has_ema else ["off"]
    if only:
        modes = [k for k in modes if k in only]
    cfg = vit.data.CONFIGS[model]
    m = vit.ViT(cfg, B, vit.VIT_FP8 if dtype == "fp8" else vit.VIT_BF16)
    m.set_params(vit.data.init_params(cfg, "ref", seed=1337))
    px, lab = vit.data.synthetic_batch(cfg, B, seed=1337)
    m.set_batch(px, lab)

    def apply(mode):
        if mode == "off":
            return  # (never set, or switched off again: the arena stays allocated, nothing touches it)
        m.set_ema(DECAY)
        m.set_option("ema_fused", int(mode == "fused"))

    def leave(mode):
        if mode != "off":
            m.set_ema(0)
            m.set_option("ema_fused", 1)

    def step():
        if opt == "sgd":
            m.train_step(1e-4)
        else:
            m.zero_grad()
            m.forward_async()
            m.backward()
            m.optimizer_step_adamw(1e-4, weight_decay=0.05)

    res = {k: [] for k in modes}
    for k in modes:  # warm every mode once
        apply(k)
        step()
        m.sync()
        leave(k)
    for _ in range(rounds):
        for k in modes:
            apply(k)
            step()
            m.sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            m.sync()
            res[k].append((time.perf_counter() - t0) / steps * 1e3)
            leave(k)
    vit.check(case)
    off = float(np.median(res["off"])) if "off" in res else float("nan")
    tag = "" if has_ema else " [other build]"
    for k in modes:
        a = np.array(res[k])
        med = float(np.median(a))
        print(f"RESULT {case:24s} {k + tag:24s} median {med:8.3f} ms/step  min {a.min():8.3f}  max {a.max():8.3f}  "
              f"vs off {100 * (med - off) / off:+6.2f} %  ({rounds} rounds x {steps} steps)", flush=True)
        print(f"rounds {case} {k + tag}: " + " ".join(f"{x:.2f}" for x in a), flush=True)  # (drift over the process)
    m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--case")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--other-lib")
    ap.add_argument("--modes", help="comma list: only these modes")
    ap.add_argument("--repeats", type=int, default=2, help="processes per case (of this build)")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.case:
        run_case(a.case, a.rounds, a.steps, a.modes.split(",") if a.modes else None)
        return 0
    lines = []
    for case in a.cases.split(","):
        libs = [None] * a.repeats
        if a.other_lib:  # this build, the other, this again
            libs.insert(1, a.other_lib)
        for lib in libs:
            env = dict(os.environ)
            if lib:
                env["VIT_LIB"] = os.path.abspath(lib)
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--case", case,
                   "--rounds", str(a.rounds), "--steps", str(a.steps)] + (["--modes", a.modes] if a.modes else [])
            r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            print(r.stdout, end="", flush=True)
            if r.returncode != 0:
                print(f"bench_ema: case {case} ended with status {r.returncode}; stopping", flush=True)
                return r.returncode
            lines += [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
