"""Cost of stochastic depth in the full step: same-process A/B of ms/step for
  off     no table ever set (the launches of a trainer without the feature),
  ones    an all-ones table set before every step (the row-scaled epilogues and the scaled planes, the
          bits of `off`),
  drawn   vit_drop_path_draw at rate 0.1 (linear over the layers), a new key every step, set before
          every step: what a training loop does (the host draw is inside the timed region).

The modes are interleaved round by round (cdna_hip_programming.md §5.4 rule 24); wall clock over
`--steps` fused train steps after a sync; the median over the rounds is reported with the spread.
Case: vit_b16 B=256 bf16.  Every case runs in a child process of its own under `timeout`, twice; the
first failure ends the run.

    python tools/bench_droppath.py [--rounds 5 --steps 10] [--out profiles/drop_path_ab.txt]
    python tools/bench_droppath.py --other-lib PATH   # + the `off` step of another build of the library
                                                      #   (e.g. the parent commit's) between the two
    python tools/bench_droppath.py --case vit_b16:256:bf16   # one case, in this process"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ["vit_b16:256:bf16"]
MODES = ["off", "ones", "drawn"]
RATE = 0.1


def run_case(case, rounds, steps, only=None):
    from vitpkg import vit
    model, batch, dtype = case.split(":")
    B = int(batch)
    L = vit.lib()
    assert L.vit_init(0) == 0
    has_dp = hasattr(L, "vit_trainer_set_drop_path")
    modes = MODES if has_dp else ["off"]
    if only:
        modes = [k for k in modes if k in only]
    cfg = vit.data.CONFIGS[model]
    m = vit.ViT(cfg, B, vit.VIT_FP32 if dtype == "fp32" else vit.VIT_BF16)
    m.set_params(vit.data.init_params(cfg, "ref", seed=1337))
    px, lab = vit.data.synthetic_batch(cfg, B, seed=1337)
    m.set_batch(px, lab)
    ones = np.ones((cfg.num_layers, 2, B), np.float32)
    dp = vit.droppath.DropPath(RATE, linear=True, seed=1337) if has_dp else None
    count = [0]

    def step(mode):
        if mode == "ones":
            m.set_drop_path(ones)
        elif mode == "drawn":
            count[0] += 1
            dp.apply(m, count[0])
        m.train_step(1e-4)

    res = {k: [] for k in modes}
    for k in modes:  # warm every mode once (the first table allocates the extra buffers)
        step(k)
        m.sync()
    for _ in range(rounds):
        for k in modes:
            step(k)
            m.sync()
            t0 = time.perf_counter()
            for _ in range(steps):
                step(k)
            m.sync()
            res[k].append((time.perf_counter() - t0) / steps * 1e3)
    vit.check(case)
    off = float(np.median(res["off"]))
    tag = "" if has_dp else " [other build]"
    for k in modes:
        a = np.array(res[k])
        med = float(np.median(a))
        print(f"RESULT {case:20s} {k + tag:20s} median {med:8.3f} ms/step  min {a.min():8.3f}  max {a.max():8.3f}  "
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
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.case:
        run_case(a.case, a.rounds, a.steps, a.modes.split(",") if a.modes else None)
        return 0
    lines = []
    for case in a.cases.split(","):
        for lib in ([None, a.other_lib, None] if a.other_lib else [None, None]):  # this build, the other, this again
            env = dict(os.environ)
            if lib:
                env["VIT_LIB"] = os.path.abspath(lib)
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--case", case,
                   "--rounds", str(a.rounds), "--steps", str(a.steps)] + (["--modes", a.modes] if a.modes else [])
            r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            print(r.stdout, end="", flush=True)
            if r.returncode != 0:
                print(f"bench_droppath: case {case} ended with status {r.returncode}; stopping", flush=True)
                return r.returncode
            lines += [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
