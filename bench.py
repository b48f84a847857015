#!/usr/bin/env python3
"""Benchmark: ViT-B/16 224x224 bf16 training step (forward + backward + SGD) on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--model vit_b16] [--batch 256] [--dtype bf16]
                    [--dump-outputs DIR] [--full]
    torchrun --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W
Run directly with --gpus N > 1 (no WORLD_SIZE in the environment) it launches the N ranks itself:
N child processes with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT set, started
before this process touches the GPU (it never does); it prints rank 0's JSON line and exits
non-zero if any rank fails.

One process per GPU.  Each rank trains on its own 256-image shard of one seeded synthetic stream
(weak scaling); gradients are summed by RCCL inside libvit_hip.so (per-layer chunks on a side
stream, overlapped with backward).  torch is used only as plumbing: the gloo process group for
the rendezvous / barrier / max-over-ranks timing and torch.cuda.synchronize(); torch is imported
BEFORE the library so the process has a single HIP runtime.

Prints ONE JSON line (rank 0).  `value` = images/s of the whole job = N*B*K / max-over-ranks
wall time of the K timed steps; `ms_per_step` = that wall time / K.  A plain run does only this:
set up, W warm-up steps, the K timed steps, the line.

--dump-outputs DIR writes (rank 0, after the timed steps) what the last timed step left for the
caller of ViT.train_step, as float32 DIR/<name>.npy: `loss` (mean_loss of its forward), `logits`
[B, classes], and `grads` / `params` (after the SGD update) at DUMP_SAMPLE canonical positions
drawn once from a fixed seed (`sample_index.npy`, float64; every position if the model is
smaller).  Inputs and parameters are seeded, so two builds run with the same arguments are
comparable array for array.

--full adds the side measurements (each a pass of its own, outside the timed region):
`loss_after_warmup` (one extra forward), `roofline` / `kernels` (the dominant GEMM class and the
per-kernel breakdown, timed with HIP events on the stream each kernel runs on, over a second pass
of the same K steps with stream concurrency off), `input_pipeline` (the same steps fed by the
native loader) and `cpu_baseline` (the CPU oracle: the reference loops restated in C, single
thread, timed on this host on a bounded sample).  --no-timing / --no-pipeline / --no-cpu-baseline
drop single legs of a --full run.
"""
import argparse
import json
import os
import sys
import time

import socket
import subprocess

import torch  # noqa: F401  (first: owns the HIP runtime of the process; importing it starts no GPU work)
import torch.distributed as dist
import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
vit = None  # vitpkg.vit, imported in the rank processes only (launch_ranks never loads the library)

METRIC = "images/sec (train step) ViT-B/16 224² bf16 at 1/2/4/8 MI355X; % MFMA roofline"
PEAK_BF16_TFLOPS = 2500.0   # MI355X dense bf16 MFMA (MI355X_MICROARCH.md chip table)
PEAK_FP8_TFLOPS = 5000.0    # dense fp8 (block-scaled f8f6f4 MFMA), same table
MODEL_NAMES = {"vit_tiny16": "ViT-Tiny/16", "vit_b16": "ViT-B/16", "vit_l16": "ViT-L/16", "vit_h14": "ViT-H/14"}
# GEMM classes that run on MXFP8 operands in --dtype fp8 (forward and input-gradient GEMMs)
FP8_CLASSES = {"gemm_qkv_fwd", "gemm_proj_fwd", "gemm_fc_fwd", "gemm_fcproj_fwd",
               "gemm_qkv_dgrad", "gemm_proj_dgrad", "gemm_fc_dgrad", "gemm_fcproj_dgrad"}
PEAK_HBM_GBS = 8000.0
DUMP_SAMPLE = 1 << 21       # --dump-outputs: canonical positions of grads / params kept (8 MiB each,
                            # 16 MiB of indices: under 64 MB in all with the logits)
DUMP_SEED = 20240229


def pmc_traffic(kernel_class):
    """HBM bytes per launch of `kernel_class` from the newest committed PMC summary
    (profiles/<tag>_traffic.json, written by tools/summarize_profile.py from separate
    rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this bench; FETCH_SIZE x 2 on gfx950).
    PMC counters cannot be read from inside a timed run, so this is the latest profiled
    measurement of the same kernel, named by its source file in `traffic_source`."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_traffic.json")))
    for f in reversed(files):
        try:
            d = json.load(open(f))
        except (OSError, ValueError):
            continue
        c = d.get("classes", {}).get(kernel_class)
        if c:
            return c["bytes_per_dispatch"], os.path.relpath(f, ROOT)
    return None, None


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model", default="vit_b16")
    ap.add_argument("--batch", type=int, default=256, help="images per GPU")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp8"],
                    help="fp8: MXFP8 forward / input-gradient GEMMs (BASELINE config 5)")
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--no-overlap", action="store_true", help="one all-reduce after backward")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's loss, logits and a seeded sample of grads / params "
                         "to DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run the side measurements: loss after warm-up, per-kernel timing / roofline "
                         "pass, input-pipeline rate, CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU oracle timing")
    ap.add_argument("--no-timing", action="store_true", help="--full without the per-kernel HIP events pass")
    ap.add_argument("--no-pipeline", action="store_true",
                    help="--full without the side measurement with the uint8 input pipeline in the loop")
    ap.add_argument("--serial", action="store_true",
                    help="run every pass with stream concurrency off (the profile command of the "
                         "per-kernel roofline pass)")
    return ap.parse_args()


def _block_once(o, t):
    """One transformer block forward + backward, in train_vit.rs:236-245 / :359-368 order."""
    B, T, C, NH, BTC = t["B"], t["T"], t["C"], t["NH"], t["BTC"]
    a, w, bv, g, gw, gb = t["a"], t["w"], t["b"], t["g"], t["gw"], t["gb"]
    x, lnw, lnb, m1, r1, m2, r2, dres = t["x"], t["lnw"], t["lnb"], t["m1"], t["r1"], t["m2"], t["r2"], t["dres"]
    for arr in list(g.values()) + list(gw.values()) + list(gb.values()) + [dres]:
        arr[:] = 0
    g["r3"][:] = t["dr3"]
    t0 = time.perf_counter()
    o.call("layernorm_forward", a["ln1"], m1, r1, x, lnw, lnb, B, T, C)
    o.call("matmul_forward", a["qkv"], a["ln1"], w["qkvw"], bv["qkvb"], B, T, C, 3 * C)
    o.call("attention_forward", a["atty"], a["pre"], a["att"], a["qkv"], B, T, C, NH)
    o.call("matmul_forward", a["proj"], a["atty"], w["projw"], bv["projb"], B, T, C, C)
    o.call("residual_forward", a["r2"], x, a["proj"], BTC)
    o.call("layernorm_forward", a["ln2"], m2, r2, a["r2"], lnw, lnb, B, T, C)
    o.call("matmul_forward", a["fch"], a["ln2"], w["fcw"], bv["fcb"], B, T, C, 4 * C)
    o.call("gelu_forward", a["fchg"], a["fch"], 4 * BTC)
    o.call("matmul_forward", a["fcp"], a["fchg"], w["fcpw"], bv["fcpb"], B, T, 4 * C, C)
    o.call("residual_forward", a["r3"], a["r2"], a["fcp"], BTC)
    dlnw, dlnb = t["dlnw"], t["dlnb"]
    o.call("residual_backward", g["r2"], g["fcp"], g["r3"], BTC)
    o.call("matmul_backward", g["fchg"], gw["fcpw"], gb["fcpb"], g["fcp"], a["fchg"], w["fcpw"], B, T, 4 * C, C)
    o.call("gelu_backward", g["fch"], a["fch"], g["fchg"], 4 * BTC)
    o.call("matmul_backward", g["ln2"], gw["fcw"], gb["fcb"], g["fch"], a["ln2"], w["fcw"], B, T, C, 4 * C)
    o.call("layernorm_backward", g["r2"], dlnw, dlnb, g["ln2"], a["r2"], lnw, m2, r2, B, T, C)
    o.call("residual_backward", dres, g["proj"], g["r2"], BTC)
    o.call("matmul_backward", g["atty"], gw["projw"], gb["projb"], g["proj"], a["atty"], w["projw"], B, T, C, C)
    o.call("attention_backward", g["qkv"], g["pre"], g["att"], g["atty"], a["qkv"], a["att"], B, T, C, NH)
    o.call("matmul_backward", g["ln1"], gw["qkvw"], gb["qkvb"], g["qkv"], a["ln1"], w["qkvw"], B, T, C, 3 * C)
    o.call("layernorm_backward", dres, dlnw, dlnb, g["ln1"], x, lnw, m1, r1, B, T, C)
    return time.perf_counter() - t0


def _cpu_model():
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return None


def config1_step(oc, o):
    """BASELINE config 1 on the CPU: one full ViT-Tiny/16 224x224 B=8 training step (forward +
    backward + SGD) of the C oracle (train_vit.rs:188-373, 737-743 restated), seeded inputs."""
    cfg = vit.data.CONFIGS["vit_tiny16"]
    B = 8
    params = o.arr(vit.data.init_params(cfg, "ref", seed=1337))
    px, lab = vit.data.synthetic_batch(cfg, B, seed=1337)
    m = oc.RefViT(o, oc.VitConfig(cfg.img, cfg.patch, cfg.in_ch, cfg.channels, cfg.num_layers,
                                  cfg.num_heads, cfg.num_classes), B)
    g = np.zeros_like(params)
    t0 = time.perf_counter()
    loss = m.forward(params, px, lab)
    m.backward(params, g)
    params -= np.float32(1e-4) * g   # optimizer_step (SGD)
    dt = time.perf_counter() - t0
    return {"model": "vit_tiny16", "batch": B, "s_per_step": round(dt, 3),
            "images_per_s": round(B / dt, 4), "loss": round(loss, 4),
            "gflop_per_step": round(B * cfg.train_gflop_per_image()[1], 2)}


def cpu_baseline(cfg, reps=3):
    """Time the CPU oracle (reference loops restated in C, 1 thread pinned to one core) on the
    GPU box's host:
      value: the bench's workload (cfg, one image) on a bounded sample — one transformer block
             forward + backward (all layer ops in train_vit.rs order, mean of `reps`) x L plus the
             patch embedding and head; images/s = 1 / (L * t_block + t_embed_head);
      config1_vit_tiny16_b8: one full ViT-Tiny/16 B=8 training step (BASELINE config 1)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_ctypes as oc
    o = oc.Oracle("f32")
    # The oracle is built with OpenMP (test speed); libgomp sized its team from the whole
    # affinity mask at load, so pin the team to one thread before timing (r03 ran a 256-thread
    # team on one core and measured 3.4x too slow).
    nth = o.set_num_threads(1)
    assert nth == 1, f"oracle OpenMP team is {nth} threads, cpu_baseline needs 1"
    allowed = os.sched_getaffinity(0)
    core = min(allowed)
    os.sched_setaffinity(0, {core})
    try:
        res = _cpu_baseline_pinned(oc, o, cfg, reps)
        res["config1_vit_tiny16_b8"] = config1_step(oc, o)
    finally:
        os.sched_setaffinity(0, allowed)
    res.update({"pinned_core": core, "cpu_model": _cpu_model(), "nproc": os.cpu_count(),
                "affinity_cpus": len(allowed)})
    return res


def _cpu_baseline_pinned(oc, o, cfg, reps):
    rng = np.random.default_rng(0)
    C, T, NH, NC, P, IMG = cfg.channels, cfg.T, cfg.num_heads, cfg.num_classes, cfg.patch, cfg.img
    B = 1
    BTC = B * T * C
    f = lambda n, s=1.0: o.arr(rng.normal(size=n) * s)
    z = lambda n: o.arr(np.zeros(n))
    acts = {k: z(n) for k, n in (("ln1", BTC), ("qkv", 3 * BTC), ("atty", BTC), ("pre", B * T * NH * T),
                                ("att", B * T * NH * T), ("proj", BTC), ("r2", BTC), ("ln2", BTC),
                                ("fch", 4 * BTC), ("fchg", 4 * BTC), ("fcp", BTC), ("r3", BTC))}
    w = {k: f(n, 0.02) for k, n in (("qkvw", 3 * C * C), ("projw", C * C), ("fcw", 4 * C * C), ("fcpw", 4 * C * C))}
    bv = {k: f(n, 0.02) for k, n in (("qkvb", 3 * C), ("projb", C), ("fcb", 4 * C), ("fcpb", C))}
    t = {"B": B, "T": T, "C": C, "NH": NH, "BTC": BTC, "a": acts, "w": w, "b": bv,
         "g": {k: z(v.size) for k, v in acts.items()}, "gw": {k: z(v.size) for k, v in w.items()},
         "gb": {k: z(v.size) for k, v in bv.items()}, "x": f(BTC), "lnw": o.arr(np.ones(C)), "lnb": z(C),
         "m1": z(B * T), "r1": z(B * T), "m2": z(B * T), "r2": z(B * T), "dres": z(BTC), "dr3": f(BTC),
         "dlnw": z(C), "dlnb": z(C)}
    t_block = sum(_block_once(o, t) for _ in range(reps)) / reps
    # patch embedding + head (forward + backward) for the same image
    K = 3 * P * P
    px = f(3 * IMG * IMG)
    pw, pb, cls, wpe = f(C * K, 0.02), z(C), z(C), z(T * C)
    enc = z(BTC)
    hw, hb = f(NC * C, 0.02), z(NC)
    logits, probs, losses = z(NC), z(NC), z(1)
    tgt = np.zeros(1, np.int32)
    lnw, lnb = t["lnw"], t["lnb"]
    t0 = time.perf_counter()
    o.call("patch_embed_forward", enc, px, pw, pb, cls, wpe, B, IMG, P, C)
    lnf, mf, rf = z(C), z(1), z(1)
    o.call("layernorm_forward", lnf, mf, rf, enc[:C].copy(), lnw, lnb, 1, 1, C)
    o.call("matmul_forward", logits, lnf, hw, hb, 1, 1, C, NC)
    o.call("softmax_forward", probs, logits, 1, 1, NC)
    o.call("crossentropy_forward", losses, probs, tgt, 1, 1, NC)
    dlog, dl = z(NC), o.arr(np.ones(1))
    o.call("crossentropy_softmax_backward", dlog, dl, probs, tgt, 1, 1, NC)
    dlnf, dhw, dhb = z(C), z(NC * C), z(NC)
    o.call("matmul_backward", dlnf, dhw, dhb, dlog, lnf, hw, 1, 1, C, NC)
    denc = f(BTC)
    o.call("patch_embed_backward", z(C * K), z(C), z(C), z(T * C), denc, px, B, IMG, P, C)
    t_rest = time.perf_counter() - t0
    t_img = cfg.num_layers * t_block + t_rest
    return {"value": round(1.0 / t_img, 5), "unit": "images/s", "cores": 1, "kind": "port",
            "sample": (f"1 image: one {cfg.name} transformer block fwd+bwd (mean of {reps}: {t_block:.2f} s) "
                       f"x {cfg.num_layers} layers + patch-embed/head fwd+bwd ({t_rest:.2f} s); "
                       f"oracle/oracle.c -O2 -ffp-contract=off, single thread")}


def pipeline_rate(m, cfg, B, args):
    """images/s of train steps whose batches come through vit.Loader -> set_batch_u8 (the
    PCIe-inclusive rate of DESIGN.md; uint8 records, 2 batches' worth in a temp file)."""
    import tempfile
    d = tempfile.mkdtemp(prefix="vit_bench_")
    try:
        n = 2 * B
        rng = np.random.default_rng(0)
        rng.integers(0, 256, size=(n, cfg.img, cfg.img, 3), dtype=np.uint8).tofile(os.path.join(d, "i.u8"))
        rng.integers(0, cfg.num_classes, size=n, dtype=np.int32).tofile(os.path.join(d, "l.i32"))
        ld = vit.Loader(os.path.join(d, "i.u8"), os.path.join(d, "l.i32"), cfg.img, B, seed=1, pinned=True)

        def step():
            ip, lp, _, _ = ld.next_raw()
            m.set_batch_u8(ip, lp)
            m.train_step(args.lr, B)

        for _ in range(2):
            step()
        m.sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        m.sync()
        dt = time.perf_counter() - t0
        ld.close()
        return {"value": round(B * args.steps / dt, 2), "unit": "images/s",
                "ms_per_step": round(dt / args.steps * 1e3, 3),
                "what": "loader (mmap, pinned 3-slot ring, 1 thread) + uint8 upload on a copy stream + "
                        "device normalise + train step, per step"}
    finally:
        for f in os.listdir(d):
            os.remove(os.path.join(d, f))
        os.rmdir(d)


def dump_outputs(m, path):
    """The arrays a caller of train_step can read back after the last timed step -> path/<name>.npy."""
    os.makedirs(path, exist_ok=True)
    n = m.num_parameters
    if n > DUMP_SAMPLE:
        idx = np.sort(np.random.default_rng(DUMP_SEED).integers(0, n, size=DUMP_SAMPLE))
    else:
        idx = np.arange(n)
    loss = float(vit.lib().vit_trainer_mean_loss(m.h))
    vit.check("mean_loss")
    np.save(os.path.join(path, "loss.npy"), np.array([loss], np.float32))
    np.save(os.path.join(path, "logits.npy"), m.logits())
    np.save(os.path.join(path, "grads.npy"), m.grads()[idx])
    np.save(os.path.join(path, "params.npy"), m.params()[idx])
    np.save(os.path.join(path, "sample_index.npy"), idx.astype(np.float64))


def _free_port():
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def launch_ranks(n):
    """Single-node launcher for `python bench.py --gpus N`: one child per GPU (the torchrun
    environment contract), this process stays off the GPU; rank 0's stdout is the result."""
    port = str(_free_port())
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL))
    out0 = procs[0].communicate()[0]
    rcs = [procs[0].returncode] + [p.wait() for p in procs[1:]]
    if out0:
        sys.stdout.write(out0.decode())
        sys.stdout.flush()
    bad = [(r, rc) for r, rc in enumerate(rcs) if rc != 0]
    if bad:
        print(f"[bench] ranks failed (rank, exit code): {bad}", file=sys.stderr)
        return 1
    return 0


def main():
    global vit
    args = parse()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(launch_ranks(args.gpus))
    from vitpkg import vit as _vit
    vit = _vit
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and rank == 0:
        print(f"[bench] note: --gpus {args.gpus} but WORLD_SIZE={world}; using WORLD_SIZE", file=sys.stderr)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo", rank=rank, world_size=world)
    L = vit.lib()
    if L.vit_init(local):
        vit.check("vit_init")
    cfg = vit.data.CONFIGS[args.model]
    B = args.batch
    m = vit.ViT(cfg, B, vit.VIT_FP8 if args.dtype == "fp8" else vit.VIT_BF16, device=local)
    m.set_params(vit.data.init_params(cfg, "ref", seed=1337))
    px, lab = vit.data.synthetic_batch(cfg, B, seed=1337, offset_images=rank * B)
    m.set_batch(px, lab)
    del px
    if world > 1:
        uid = [vit.ViT.dp_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(uid, src=0)
        m.dp_init(rank, world, uid[0], overlap=not args.no_overlap)
    rccl_ranks = m.dp_ranks()  # ncclCommCount of the trainer's communicator (0 = no DP)
    b_global = B * world
    if args.serial:
        m.set_concurrency(False)

    for _ in range(args.warmup):
        m.train_step(args.lr, b_global)
    m.sync()
    # --full sanity: finite loss after warmup (one extra forward)
    loss_w = m.forward() if args.full and args.warmup else None

    def timed(steps):
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(local)
        m.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            m.train_step(args.lr, b_global)
        m.sync()
        torch.cuda.synchronize(local)
        if world > 1:
            dist.barrier()
        dt = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([dt], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        return dt

    # the timed region: K plain steps with the production stream concurrency (two micro-batch
    # streams + the weight-gradient stream) and no per-kernel events (~3 % of a step)
    dt = timed(args.steps)
    if args.dump_outputs and rank == 0:
        dump_outputs(m, args.dump_outputs)
    # then the same K steps again, kernels one at a time (concurrency off), with HIP events
    # around every kernel class: the per-kernel breakdown and the roofline of the dominant kernel
    # (durations of kernels that share the GPU with another stream's kernels mean nothing)
    kern = {}
    if args.full and not args.no_timing:
        m.set_concurrency(False)
        timed(1)
        m.timing_reset()
        m.set_timing(True)
        timed(args.steps)
        m.set_timing(False)
        kern = m.timing()
    # side measurement (N=1, not `value`): the same steps fed by the input pipeline — the native
    # loader (pinned ring, background thread) + uint8 H2D upload + device normalise in the loop
    pipe = None
    if args.full and world == 1 and not args.no_pipeline:
        m.set_concurrency(not args.serial)
        pipe = pipeline_rate(m, cfg, B, args)
    ips = world * B * args.steps / dt
    _, gflop_img = cfg.train_gflop_per_image()

    out = None
    if rank == 0:
        def roofline(classes, peak):
            gemms = {k: v for k, v in kern.items() if k in classes}
            if not gemms:
                return None
            dom = max(gemms, key=lambda k: gemms[k]["ms"])
            d = gemms[dom]
            avg_ms = d["ms"] / d["calls"]
            ach = d["flops"] / d["calls"] / (avg_ms * 1e-3) / 1e12
            # the committed PMC passes profile the default workload (ViT-B/16 bf16, B=256); other
            # models / dtypes have no traffic measurement of their own
            traffic, tsrc = (pmc_traffic(dom) if args.model == "vit_b16" and args.dtype == "bf16"
                             and B == 256 else (None, None))
            return {"kernel": dom, "bound": "mfma", "achieved": round(ach, 1), "peak": peak,
                    "unit": "TFLOP/s", "frac": round(ach / peak, 4),
                    "traffic": round(traffic) if traffic else None, "traffic_unit": "bytes/launch",
                    "traffic_source": tsrc,
                    "avg_launch_ms": round(avg_ms, 4), "flops_per_launch": d["flops"] / d["calls"]}
        all_gemms = {k for k in kern if k.startswith("gemm_")}
        if args.dtype == "fp8":
            roof = roofline(all_gemms & FP8_CLASSES, PEAK_FP8_TFLOPS)
            roof_bf16 = roofline(all_gemms - FP8_CLASSES, PEAK_BF16_TFLOPS)
        else:
            roof, roof_bf16 = roofline(all_gemms, PEAK_BF16_TFLOPS), None
        ksum = {k: {"ms_per_step": round(v["ms"] / args.steps, 3), "calls_per_step": v["calls"] // args.steps,
                    "tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 1) if v["flops"] and v["ms"] else None}
                for k, v in sorted(kern.items(), key=lambda kv: -kv[1]["ms"])}
        metric = METRIC
        step_peak = PEAK_FP8_TFLOPS if args.dtype == "fp8" else PEAK_BF16_TFLOPS
        if args.model != "vit_b16" or args.dtype != "bf16":
            metric = (f"images/sec (train step) {MODEL_NAMES.get(cfg.name, cfg.name)} {cfg.img}² {args.dtype} "
                      f"on MI355X; % MFMA roofline")
        out = {
            "metric": metric, "value": round(ips, 2), "unit": "images/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype,
            "data": "synthetic (seeded splitmix64: N(0,1) pixels, uniform labels; reference init U[0,1)*0.02)",
            "rccl_ranks": rccl_ranks,
            "config": {"workload": f"{cfg.name} {cfg.img}x{cfg.img} train step (fwd+bwd+SGD), batch {B}/GPU, {args.dtype}",
                       "model": cfg.name, "global_batch": b_global, "seq_len": cfg.T,
                       "parallelism": f"dp{world}"},
            # the step's algorithmic flops against the dense peak of its GEMM dtype (fp8 mode: the
            # 5 PF fp8 peak, though attention and the weight gradients' reduce stay bf16 / fp32)
            "mfma_roofline_frac_step": round(ips * gflop_img / world / (step_peak * 1e3), 4),
            "mfma_roofline_frac_step_peak_tflops": step_peak,
            **({"mfma_roofline_frac_step_vs_bf16_peak": round(ips * gflop_img / world / (PEAK_BF16_TFLOPS * 1e3), 4)}
               if args.dtype == "fp8" else {}),
            "train_gflop_per_image": round(gflop_img, 3),
            "loss_after_warmup": round(loss_w, 4) if loss_w is not None else None,
            "full": args.full,
            "roofline": roof, "kernels": ksum,
            **({"roofline_bf16_gemms": roof_bf16, "fp8_gemm_classes": sorted(FP8_CLASSES)} if args.dtype == "fp8" else {}), "input_pipeline": pipe,
            "kernels_note": "per-kernel ms from HIP events over a second pass of the same steps run "
                            "with stream concurrency off (kernels one at a time; the weight gradients' "
                            "split-K then sized for 80 % of the slots instead of the 45 % they use "
                            "beside the micro-batch streams)",
        }
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(cfg)
    elif rank == 0:
        out["cpu_baseline"] = None
    m.close()
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
