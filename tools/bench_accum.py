"""Cost of gradient accumulation in the full step: same-process A/B of ms per micro-step
(one train_step call) for
  off        accumulation never set: every call updates (the step of a trainer without the feature),
  plain      N micro-steps per window, option accum_overlap = 0: one summing launch behind each backward,
  overlap    the same with accum_overlap = 1: the sums per gradient chunk on the side stream,
  off_late   (fp8 only) accumulation off with early_sgd = 0: what fp8 pays for its early per-chunk SGD, which
             N - 1 of N micro-steps cannot take, apart from the summing pass itself,
and the summing kernel alone (the grad_accumulate op on the model's arena size) in TB/s next to the
ema_update op, which moves the same 12 B per element, in the same process.

The modes are applied between steps and interleaved round by round (cdna_hip_programming.md §5.4
rule 24); wall clock over `--steps` train_step calls (a multiple of N) after a sync; the median over the
rounds is reported with the spread.  Cases: vit_b16 B=256 bf16, vit_h14 B=128 fp8.  Every case runs in a
child process of its own under `timeout`, twice; the first failure ends the run.

    python tools/bench_accum.py [--rounds 5 --steps 12 --accum 4] [--out profiles/grad_accum_ab.txt]
    python tools/bench_accum.py --other-lib PATH   # + the `off` step of another build of the library
                                                   #   (e.g. the parent commit's) between the two
    python tools/bench_accum.py --case vit_b16:256:bf16   # one case, in this process"""
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
MODES = ["off", "plain", "overlap", "off_late"]


def kernel_alone(vit, n, rounds, launches=20):
    """GB/s of grad_accumulate (in place, as the trainer runs it) and of ema_update over n floats: `launches`
    launches between two events on the context stream, interleaved round by round"""
    L = vit.lib()
    bufs = [vit.DeviceArray.zeros(n, np.float32) for _ in range(2)]
    e0, e1 = L.vit_event_create(), L.vit_event_create()

    def timed(fn):
        fn()
        L.vit_sync()
        L.vit_event_record(e0)
        for _ in range(launches):
            fn()
        L.vit_event_record(e1)
        L.vit_sync()
        return L.vit_event_elapsed_ms(e0, e1) / launches

    ops = {"grad_accumulate": lambda: L.grad_accumulate(bufs[0].ptr, bufs[0].ptr, bufs[1].ptr, n),
           "ema_update": lambda: L.ema_update(bufs[0].ptr, bufs[1].ptr, n, 0.9999)}
    res = {k: [] for k in ops}
    for _ in range(rounds):
        for k, fn in ops.items():
            res[k].append(timed(fn))
    vit.check("kernel_alone")
    for b in bufs:
        b.free()
    L.vit_event_destroy(e0)
    L.vit_event_destroy(e1)
    return {k: np.array(v) for k, v in res.items()}


def run_case(case, rounds, steps, accum, only=None):
    from vitpkg import vit
    model, batch, dtype = case.split(":")
    B = int(batch)
    L = vit.lib()
    assert L.vit_init(0) == 0
    has_accum = hasattr(L, "vit_trainer_set_grad_accum")
    modes = [k for k in MODES if k != "off_late" or dtype == "fp8"] if has_accum else ["off"]
    if only:
        modes = [k for k in modes if k in only]
    assert steps % accum == 0, "--steps must be a multiple of --accum"
    cfg = vit.data.CONFIGS[model]
    m = vit.ViT(cfg, B, vit.VIT_FP8 if dtype == "fp8" else vit.VIT_BF16)
    m.set_params(vit.data.init_params(cfg, "ref", seed=1337))
    px, lab = vit.data.synthetic_batch(cfg, B, seed=1337)
    m.set_batch(px, lab)

    def apply(mode):
        if mode == "off_late":
            m.set_option("early_sgd", 0)
        if mode in ("plain", "overlap"):
            m.set_option("accum_overlap", int(mode == "overlap"))
            m.set_grad_accum(accum)

    def leave(mode):
        if mode == "off_late":
            m.set_option("early_sgd", -1)
        if mode in ("plain", "overlap"):
            m.set_grad_accum(1)
            m.set_option("accum_overlap", -1)

    def window():  # `accum` calls: one whole window, or that many plain steps
        for _ in range(accum):
            m.train_step(1e-4)

    res = {k: [] for k in modes}
    for k in modes:  # warm every mode once (the accumulator is allocated here)
        apply(k)
        window()
        m.sync()
        leave(k)
    for _ in range(rounds):
        for k in modes:
            apply(k)
            window()
            m.sync()
            t0 = time.perf_counter()
            for _ in range(steps // accum):
                window()
            m.sync()
            res[k].append((time.perf_counter() - t0) / steps * 1e3)
            leave(k)
    vit.check(case)
    off = float(np.median(res["off"])) if "off" in res else float("nan")
    tag = "" if has_accum else " [other build]"
    for k in modes:
        a = np.array(res[k])
        med = float(np.median(a))
        print(f"RESULT {case:18s} {k + tag:22s} median {med:8.3f} ms/micro-step  min {a.min():8.3f}  max {a.max():8.3f}  "
              f"vs off {100 * (med - off) / off:+6.2f} %  (N = {accum if k in ('plain', 'overlap') else 1}, "
              f"{rounds} rounds x {steps} calls)", flush=True)
        print(f"rounds {case} {k + tag}: " + " ".join(f"{x:.2f}" for x in a), flush=True)  # (drift over the process)
    m.close()
    if has_accum and not only:
        n = ctypes.c_longlong()
        assert L.vit_layout_query(ctypes.byref(vit._cfg_c(cfg)), None, None, ctypes.byref(n)) > 0
        n = n.value
        for k, a in kernel_alone(vit, n, rounds).items():
            med = float(np.median(a))
            print(f"RESULT {case:18s} {'op ' + k:22s} median {med * 1e3:8.1f} us  min {a.min() * 1e3:8.1f}  max "
                  f"{a.max() * 1e3:8.1f}  {12 * n / med / 1e9:6.2f} TB/s at the median  (n = {n}, 12 B per element)",
                  flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--accum", type=int, default=4)
    ap.add_argument("--case")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--other-lib")
    ap.add_argument("--modes", help="comma list: only these modes")
    ap.add_argument("--repeats", type=int, default=2, help="processes per case (of this build)")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.case:
        run_case(a.case, a.rounds, a.steps, a.accum, a.modes.split(",") if a.modes else None)
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
                   "--rounds", str(a.rounds), "--steps", str(a.steps), "--accum", str(a.accum)]
            cmd += ["--modes", a.modes] if a.modes else []
            r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            print(r.stdout, end="", flush=True)
            if r.returncode != 0:
                print(f"bench_accum: case {case} ended with status {r.returncode}; stopping", flush=True)
                return r.returncode
            lines += [ln[7:] for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
