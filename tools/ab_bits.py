"""Same bits across two builds: a fixed list of small training cases over the trainer's modes and options.
    python tools/ab_bits.py run --out new.npz [--only NAME[,NAME..]]
    VIT_LIB=ab/parent/libvit_hip.so python tools/ab_bits.py run --out parent.npz
    python tools/ab_bits.py compare parent.npz new.npz        # exits 1 if any array differs
Uses only the Python API, so VIT_LIB can point it at an older build.  Each case builds a fresh trainer (fixed
seeds, concurrency on unless the case says otherwise) and stores, after one zero_grad / forward / backward, the
loss, logits, gradients and the whole kernel_hits vector, and after two further train_steps the logits and
parameters.  The fp8 cases assert that they take the MX paths they are there for."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vitpkg import vit  # noqa: E402

H64 = vit.data.CONFIGS["test_h64"]  # C = 128, T = 17, L = 2
# the geometry of tests/test_gpu_last_cls_bwd.py (T = 197): B = 32 reaches the K-skip weight-gradient engine
LASTBLK = vit.data.VitCfg("prod_l2", img=224, patch=16, channels=256, num_layers=2, num_heads=4, num_classes=1000)
# T = 17, so B = 128 gives micro-batches of whole 64-token chunks: the row+column MX forms are on
FP8 = vit.data.VitCfg("fp8_l2", img=32, patch=8, channels=256, num_layers=2, num_heads=4, num_classes=10)
# K = 588 -> 640: the padded patch GEMMs
PAD = vit.data.VitCfg("pad_l1", img=56, patch=14, channels=128, num_layers=1, num_heads=2, num_classes=10)
BF16, FP8P, FP32 = vit.VIT_BF16, vit.VIT_FP8, vit.VIT_FP32


def lnb_mx_supported(C):  # gemm_fp8.hip ln_backward_mx_supported
    return C % 256 == 0 and 256 <= C <= 1280


def case(name, cfg, B, prec, opts=(), **kw):
    return dict(name=name, cfg=cfg, B=B, prec=prec, opts=dict(opts), **kw)


CASES = [case("h64_fp32", H64, 8, FP32)]
CASES += [case(f"h64_bf16_mb{n}", H64, 8, BF16, {"microbatch": n}) for n in (1, 2, 4)]
CASES += [
    case("h64_bf16_serial", H64, 8, BF16, concurrency=False),
    case("h64_bf16_timing", H64, 8, BF16, timing=True),
    case("h64_bf16_adamw", H64, 8, BF16, adamw=True),
    case("h64_bf16_early_sgd", H64, 8, BF16, {"early_sgd": 1}),
    case("h64_bf16_clip_overlap", H64, 8, BF16, {"clip_overlap": 1}, clip=0.5),
    case("h64_bf16_dp_overlap", H64, 8, BF16, dp=True),
    case("h64_bf16_dp_plain", H64, 8, BF16, dp=False),
]
CASES += [case(f"lastblk_bwd{b}", LASTBLK, 32, BF16, {"microbatch": 2, "last_cls_bwd": b}) for b in (0, 1, 2)]
CASES += [
    case("lastblk_full", LASTBLK, 32, BF16, {"microbatch": 2, "last_cls": 0}),
    case("lastblk_droppath_bwd2", LASTBLK, 32, BF16, {"microbatch": 2, "last_cls_bwd": 2}, drop=0.5),
    case("lastblk_droppath_full", LASTBLK, 32, BF16, {"microbatch": 2, "last_cls": 0}, drop=0.5),
    case("lastblk_b8", LASTBLK, 8, BF16, {"microbatch": 2}),
    case("fp8_mb1", FP8, 128, FP8P, {"microbatch": 1}, mx=True),
    case("fp8_mb2", FP8, 128, FP8P, {"microbatch": 2}, mx=True),
    case("fp8_nofuse", FP8, 128, FP8P, {"microbatch": 2}, env="VIT_FP8_FUSE"),
    case("fp8_norowcol", FP8, 128, FP8P, {"microbatch": 2}, env="VIT_FP8_ROWCOL"),
    case("fp8_nowtcols", FP8, 128, FP8P, {"microbatch": 2}, env="VIT_FP8_WT_COLS"),
    case("fp8_h64_b8", H64, 8, FP8P),
    case("pad_bf16", PAD, 8, BF16),
    case("pad_fp8", PAD, 8, FP8P),
]


def run_case(c, out):
    cfg, B = c["cfg"], c["B"]
    params = vit.data.init_params(cfg, "parity", seed=3)
    px, lab = vit.data.synthetic_batch(cfg, B, seed=5)
    if c.get("env"):  # read when the trainer is built
        os.environ[c["env"]] = "0"
    m = vit.ViT.build(cfg, B, c["prec"], params=params)
    if c.get("env"):
        del os.environ[c["env"]]
    m.set_concurrency(c.get("concurrency", True))
    for k, val in c["opts"].items():
        m.set_option(k, val)
    if c.get("timing"):
        m.set_timing(True)
    if c.get("clip"):
        m.set_grad_clip(c["clip"])
    if c.get("dp") is not None:
        m.dp_init(0, 1, vit.ViT.dp_unique_id(), overlap=c["dp"])
    if c.get("drop"):
        m.set_drop_path(vit.droppath.draw(1337, 0, cfg.num_layers, B, c["drop"]))
    vit.kernel_hits_reset()
    m.set_batch(px, lab)
    m.zero_grad()
    loss = m.forward()
    m.backward()
    m.sync()
    hits = vit.kernel_hits()
    if c.get("mx"):
        assert hits[vit.HIT_QUANT_ROWCOL] + hits[vit.HIT_LN_MX] > 0, (c["name"], "no row+column MX form ran")
        assert hits[vit.HIT_LNB_MX] > 0 or not lnb_mx_supported(cfg.channels), (c["name"], "no MX LayerNorm backward")
    n = c["name"]
    out[n + "/loss"] = np.float64(loss)
    out[n + "/logits"] = m.logits()
    out[n + "/grads"] = m.grads()
    out[n + "/kernel_hits"] = hits
    for _ in range(2):
        if c.get("adamw"):
            m.zero_grad()
            m.forward()
            m.backward()
            m.optimizer_step_adamw(1e-3, weight_decay=0.05)
        else:
            m.train_step(0.05)
    m.sync()
    out[n + "/logits2"] = m.logits()
    out[n + "/params2"] = m.params()
    m.close()
    vit.check(n)


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    bad = sorted(set(a.files) ^ set(b.files))
    for k in bad:
        print(f"only in one file: {k}")
    for k in sorted(set(a.files) & set(b.files)):
        x, y = a[k], b[k]
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            ndiff = int(np.sum(x != y)) if x.shape == y.shape else -1
            print(f"DIFF {k}: {ndiff} of {x.size} elements")
            bad.append(k)
    print(f"{len(a.files)} arrays, {len(bad)} differ")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--out", required=True)
    r.add_argument("--only", default="", help="comma-separated case names (default: all)")
    c = sub.add_parser("compare")
    c.add_argument("a")
    c.add_argument("b")
    args = ap.parse_args()
    if args.cmd == "compare":
        sys.exit(compare(args.a, args.b))
    only = set(filter(None, args.only.split(",")))
    assert only <= {c["name"] for c in CASES}, only
    assert vit.lib().vit_init(0) == 0
    out = {}
    for c in CASES:
        if only and c["name"] not in only:
            continue
        run_case(c, out)
        print(f"{c['name']}: loss {float(out[c['name'] + '/loss']):.6f}", flush=True)
    np.savez(args.out, **out)


if __name__ == "__main__":
    main()
