"""Reference ViT step with stochastic depth (test infrastructure, CPU only).

The op sequence of the oracle's ref_vit_forward / ref_vit_backward (oracle/oracle.c), composed here
from its op-level functions through oracle_ctypes.Oracle.call, with the two residual adds of each
block and their backward in numpy so that they can scale the branch per image:

    forward   x_out[r] = x_in[r] + fl(s * y[r])
    backward  d_in[r] += d_out[r];   d_branch[r] += fl(s * d_out[r])

for every row r of image b, s = scales[l][br][b] (br 0 = attention, 1 = MLP), fl = one rounding to
the oracle's precision (fp32 or fp64).  With all-ones scales the step has the bits of RefViT's.
"""
import numpy as np

import oracle_ctypes as oc


def step(o, cfg, params, pixels, targets, scales=None, b_global=None, backward=True):
    """-> (mean loss, logits [B, NC], grads flat canonical or None).  cfg: a vit.data.VitCfg (or any
    object with its fields); scales [L, 2, B] or None (all ones)."""
    dt = o.dtype
    c = oc.VitConfig(cfg.img, cfg.patch, cfg.in_ch, cfg.channels, cfg.num_layers, cfg.num_heads, cfg.num_classes)
    B = int(np.asarray(pixels).shape[0])
    C, L, NH, NC = cfg.channels, cfg.num_layers, cfg.num_heads, cfg.num_classes
    T = (cfg.img // cfg.patch) ** 2 + 1
    BT, BTC = B * T, B * T * C
    p_flat = o.arr(params)
    px = o.arr(pixels)
    tg = np.ascontiguousarray(targets, dtype=np.int32)
    s = np.ones((L, 2, B), dt) if scales is None else np.asarray(scales).astype(dt)
    assert s.shape == (L, 2, B)
    p = oc.split_params(o, c, p_flat)
    z = lambda *shape: np.zeros(shape, dt)  # noqa: E731

    def lay(d, name, l):
        n = d[name].size // L
        return d[name][l * n:(l + 1) * n]

    def rows(l, br):  # the scale of every element of a [B*T*C] tensor
        return np.repeat(s[l, br], T * C)

    enc = z(BTC)
    o.call("patch_embed_forward", enc, px, p["patch_w"], p["patch_b"], p["cls"], p["wpe"], B, cfg.img, cfg.patch, C)
    acts = []
    x = enc
    for l in range(L):
        a = dict(x=x, ln1=z(BTC), ln1_mean=z(BT), ln1_rstd=z(BT), qkv=z(3 * BTC), atty=z(BTC),
                 preatt=z(BT * NH * T), att=z(BT * NH * T), attproj=z(BTC), ln2=z(BTC), ln2_mean=z(BT),
                 ln2_rstd=z(BT), fch=z(4 * BTC), fchg=z(4 * BTC), fcproj=z(BTC))
        o.call("layernorm_forward", a["ln1"], a["ln1_mean"], a["ln1_rstd"], x, lay(p, "ln1w", l), lay(p, "ln1b", l), B, T, C)
        o.call("matmul_forward", a["qkv"], a["ln1"], lay(p, "qkvw", l), lay(p, "qkvb", l), B, T, C, 3 * C)
        o.call("attention_forward", a["atty"], a["preatt"], a["att"], a["qkv"], B, T, C, NH)
        o.call("matmul_forward", a["attproj"], a["atty"], lay(p, "attprojw", l), lay(p, "attprojb", l), B, T, C, C)
        a["res2"] = (x + (rows(l, 0) * a["attproj"]).astype(dt)).astype(dt)
        o.call("layernorm_forward", a["ln2"], a["ln2_mean"], a["ln2_rstd"], a["res2"], lay(p, "ln2w", l), lay(p, "ln2b", l), B, T, C)
        o.call("matmul_forward", a["fch"], a["ln2"], lay(p, "fcw", l), lay(p, "fcb", l), B, T, C, 4 * C)
        o.call("gelu_forward", a["fchg"], a["fch"], 4 * BTC)
        o.call("matmul_forward", a["fcproj"], a["fchg"], lay(p, "fcprojw", l), lay(p, "fcprojb", l), B, T, 4 * C, C)
        a["res3"] = (a["res2"] + (rows(l, 1) * a["fcproj"]).astype(dt)).astype(dt)
        acts.append(a)
        x = a["res3"]
    lnf, lnf_mean, lnf_rstd = z(B * C), z(B), z(B)
    for b in range(B):
        o.call("layernorm_forward", lnf[b * C:(b + 1) * C], lnf_mean[b:b + 1], lnf_rstd[b:b + 1],
               x[b * T * C:b * T * C + C], p["lnfw"], p["lnfb"], 1, 1, C)
    logits, probs, losses = z(B * NC), z(B * NC), z(B)
    o.call("matmul_forward", logits, lnf, p["head_w"], p["head_b"], B, 1, C, NC)
    o.call("softmax_forward", probs, logits, B, 1, NC)
    o.call("crossentropy_forward", losses, probs, tg, B, 1, NC)
    mean_loss = dt(0)
    for i in range(B):
        mean_loss = dt(mean_loss + losses[i])
    mean_loss = dt(mean_loss / dt(B))
    if not backward:
        return float(mean_loss), logits.reshape(B, NC), None

    g_flat = np.zeros_like(p_flat)
    g = oc.split_params(o, c, g_flat)
    dlosses = np.full(B, dt(1.0) / dt(b_global or B), dt)
    dlogits, dlnf = z(B * NC), z(B * C)
    o.call("crossentropy_softmax_backward", dlogits, dlosses, probs, tg, B, 1, NC)
    o.call("matmul_backward", dlnf, g["head_w"], g["head_b"], dlogits, lnf, p["head_w"], B, 1, C, NC)
    dres3 = z(BTC)
    for b in range(B):
        o.call("layernorm_backward", dres3[b * T * C:b * T * C + C], g["lnfw"], g["lnfb"], dlnf[b * C:(b + 1) * C],
               x[b * T * C:b * T * C + C], p["lnfw"], lnf_mean[b:b + 1], lnf_rstd[b:b + 1], 1, 1, C)
    for l in range(L - 1, -1, -1):
        a = acts[l]
        dres2, dfcproj = z(BTC), z(BTC)
        dres2 += dres3
        dfcproj += (rows(l, 1) * dres3).astype(dt)
        dfchg, dfch, dln2 = z(4 * BTC), z(4 * BTC), z(BTC)
        o.call("matmul_backward", dfchg, lay(g, "fcprojw", l), lay(g, "fcprojb", l), dfcproj, a["fchg"],
               lay(p, "fcprojw", l), B, T, 4 * C, C)
        o.call("gelu_backward", dfch, a["fch"], dfchg, 4 * BTC)
        o.call("matmul_backward", dln2, lay(g, "fcw", l), lay(g, "fcb", l), dfch, a["ln2"], lay(p, "fcw", l), B, T, C, 4 * C)
        o.call("layernorm_backward", dres2, lay(g, "ln2w", l), lay(g, "ln2b", l), dln2, a["res2"], lay(p, "ln2w", l),
               a["ln2_mean"], a["ln2_rstd"], B, T, C)
        dres, dattproj = z(BTC), z(BTC)
        dres += dres2
        dattproj += (rows(l, 0) * dres2).astype(dt)
        datty, dqkv, dpreatt, datt, dln1 = z(BTC), z(3 * BTC), z(BT * NH * T), z(BT * NH * T), z(BTC)
        o.call("matmul_backward", datty, lay(g, "attprojw", l), lay(g, "attprojb", l), dattproj, a["atty"],
               lay(p, "attprojw", l), B, T, C, C)
        o.call("attention_backward", dqkv, dpreatt, datt, datty, a["qkv"], a["att"], B, T, C, NH)
        o.call("matmul_backward", dln1, lay(g, "qkvw", l), lay(g, "qkvb", l), dqkv, a["ln1"], lay(p, "qkvw", l), B, T, C, 3 * C)
        o.call("layernorm_backward", dres, lay(g, "ln1w", l), lay(g, "ln1b", l), dln1, a["x"], lay(p, "ln1w", l),
               a["ln1_mean"], a["ln1_rstd"], B, T, C)
        dres3 = dres
    o.call("patch_embed_backward", g["patch_w"], g["patch_b"], g["cls"], g["wpe"], dres3, px, B, cfg.img, cfg.patch, C)
    return float(mean_loss), logits.reshape(B, NC), g_flat
