"""Soft-target batch mixing: the per-batch random draw (Mixer) and the numpy statement of what
vit_trainer_mix_batch and the soft-target loss compute (reference_mix, soft_targets).

Image i of a batch is paired with image B-1-i; one (mode, lam, box) holds for the whole batch.
Host-only (numpy): nothing here touches the GPU.
"""
import math

import numpy as np

MIX_NONE, MIX_MIXUP, MIX_CUTMIX = 0, 1, 2  # include/vit_trainer.h VIT_MIX_*


def cutmix_lam(box, img):
    """The label weight the library derives from a cutmix box: 1 - area / img^2 in double,
    rounded to float."""
    x0, y0, x1, y1 = box
    return float(np.float32(1.0 - float((x1 - x0) * (y1 - y0)) / (float(img) * float(img))))


class Mixer:
    """One mixup / cutmix decision per batch from a seeded numpy RandomState.

    draw(img) -> (mode, lam, box), the arguments of ViT.mix_batch:
      with probability 1 - prob                      (MIX_NONE, 1.0, None);
      cutmix with probability switch_prob when both alphas are > 0 (else whichever alpha is > 0);
      lam ~ Beta(alpha, alpha);
      mixup:  (MIX_MIXUP, lam, None);
      cutmix: a box of side ratio sqrt(1 - lam) around a uniform centre, clipped to the image,
              and the area-corrected lam the library will use: (MIX_CUTMIX, lam, (x0, y0, x1, y1)).
    """

    def __init__(self, mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, seed=0):
        self.mixup_alpha = float(mixup_alpha)
        self.cutmix_alpha = float(cutmix_alpha)
        self.prob = float(prob)
        self.switch_prob = float(switch_prob)
        self.rng = np.random.RandomState(seed)

    def draw(self, img):
        rng = self.rng
        if not rng.random_sample() < self.prob:
            return MIX_NONE, 1.0, None
        if self.mixup_alpha > 0 and self.cutmix_alpha > 0:
            cut = bool(rng.random_sample() < self.switch_prob)
        elif self.cutmix_alpha > 0:
            cut = True
        elif self.mixup_alpha > 0:
            cut = False
        else:
            return MIX_NONE, 1.0, None
        alpha = self.cutmix_alpha if cut else self.mixup_alpha
        lam = float(np.float32(min(max(rng.beta(alpha, alpha), 0.0), 1.0)))
        if not cut:
            return MIX_MIXUP, lam, None
        side = int(img * math.sqrt(1.0 - lam))
        cx, cy = int(rng.randint(img)), int(rng.randint(img))
        x0, x1 = max(cx - side // 2, 0), min(cx + side // 2, img)
        y0, y1 = max(cy - side // 2, 0), min(cy + side // 2, img)
        box = (x0, y0, x1, y1)
        return MIX_CUTMIX, cutmix_lam(box, img), box


def reference_mix(px, labels, mode, lam=1.0, box=None):
    """numpy fp32 statement of vit_trainer_mix_batch on pixels [B, 3, img, img] and labels [B]:
    -> (pixels, ta, tb, lam_used), bit for bit what the device batch holds afterwards.

    mixup:  x_i' = rn(rn(lam x_i) + rn(oml x_j)), j = B-1-i, oml = 1 - lam in fp32;
    cutmix: the box [x0,x1) x [y0,y1) of every channel plane is swapped between i and j,
            lam_used = 1 - area / img^2;
    the middle image of an odd B is its own partner and keeps its bits."""
    px = np.array(px, dtype=np.float32, copy=True)
    ta = np.asarray(labels, dtype=np.int32).copy()
    tb = ta[::-1].copy()
    B, img = px.shape[0], px.shape[-1]
    if mode == MIX_NONE:
        return px, ta, ta.copy(), 1.0
    if mode == MIX_MIXUP:
        lam32 = np.float32(lam)
        oml = np.float32(1.0) - lam32
        out = (lam32 * px).astype(np.float32) + (oml * px[::-1]).astype(np.float32)
        if B % 2:
            out[B // 2] = px[B // 2]
        return out.astype(np.float32), ta, tb, float(lam32)
    if mode == MIX_CUTMIX:
        x0, y0, x1, y1 = box
        out = px.copy()
        out[:, :, y0:y1, x0:x1] = px[::-1, :, y0:y1, x0:x1]
        return out, ta, tb, cutmix_lam(box, img)
    raise ValueError(f"unknown mix mode {mode}")


def soft_targets(ta, tb, lam, eps, V):
    """float64 [rows, V] target distributions t = (1-eps) (lam 1[ta] + oml 1[tb]) + eps/V with
    lam, eps taken as float32 and oml = 1 - lam in fp32, as the kernels take them (tb None = ta)."""
    ta = np.asarray(ta, dtype=np.int64)
    tb = ta if tb is None else np.asarray(tb, dtype=np.int64)
    lam32 = np.float32(lam)
    oml = float(np.float32(1.0) - lam32)
    e = float(np.float32(eps))
    rows = np.arange(ta.size)
    hard = np.zeros((ta.size, V), np.float64)
    hard[rows, ta] += float(lam32)
    hard[rows, tb] += oml
    return (1.0 - e) * hard + e / V
