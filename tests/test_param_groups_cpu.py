"""Host side of parameter groups (vit.rs_amd/groups.py): the weight-decay exclusion table, the
layer-wise learning-rate decay table and the expansion of the wrapper's dict / array arguments.
No GPU."""
import numpy as np
import pytest

F32 = np.float32
CFGS = ["test", "test_h64", "vit_b16"]
EMBED = ("patch_w", "patch_b", "cls", "wpe")
HEAD = ("lnfw", "lnfb", "head_w", "head_b")


def per_layer_shapes(cfg):
    """shape of one layer's (or the whole unlayered) tensor, by name, from the model's dimensions"""
    C, K, T, NC = cfg.channels, cfg.in_ch * cfg.patch ** 2, cfg.T, cfg.num_classes
    return {"patch_w": (C, K), "patch_b": (C,), "cls": (C,), "wpe": (T, C),
            "ln1w": (C,), "ln1b": (C,), "qkvw": (3 * C, C), "qkvb": (3 * C,), "attprojw": (C, C), "attprojb": (C,),
            "ln2w": (C,), "ln2b": (C,), "fcw": (4 * C, C), "fcb": (4 * C,), "fcprojw": (C, 4 * C), "fcprojb": (C,),
            "lnfw": (C,), "lnfb": (C,), "head_w": (NC, C), "head_b": (NC,)}


@pytest.mark.parametrize("name", CFGS)
def test_no_decay(vit, name):
    cfg = vit.data.CONFIGS[name]
    names, L = vit.data.PARAM_NAMES, cfg.num_layers
    shapes = per_layer_shapes(cfg)
    # the shapes above are the canonical sizes
    for n, size in zip(names, cfg.param_sizes()):
        layers = L if n in vit.data.LAYER_PARAMS else 1
        assert int(np.prod(shapes[n])) * layers == size, n
    wd = vit.groups.no_decay(cfg)
    assert wd.shape == (20, L) and wd.dtype == F32
    for ti, n in enumerate(names):
        excluded = len(shapes[n]) == 1 or n in ("cls", "wpe")
        assert np.array_equal(wd[ti], np.full(L, 0.0 if excluded else 1.0, F32)), n
    assert sorted(names[ti] for ti in range(20) if wd[ti, 0] == 1) == sorted(
        ["patch_w", "qkvw", "attprojw", "fcw", "fcprojw", "head_w"])


@pytest.mark.parametrize("name", CFGS)
def test_layer_decay(vit, name):
    cfg = vit.data.CONFIGS[name]
    names, L = vit.data.PARAM_NAMES, cfg.num_layers
    lr = vit.groups.layer_decay(cfg, 0.75)
    assert lr.shape == (20, L) and lr.dtype == F32
    for ti, n in enumerate(names):
        for l in range(L):
            lid = 0 if n in EMBED else L + 1 if n in HEAD else l + 1
            want = F32(0.75 ** (L + 1 - lid))
            assert lr[ti, l] == want, (n, l, lr[ti, l], want)
    for n in HEAD:
        assert np.all(lr[names.index(n)] == 1.0)
    for n in vit.data.LAYER_PARAMS:
        row = lr[names.index(n)]
        assert np.all(np.diff(row) > 0), n  # deeper blocks learn faster
        assert lr[names.index("patch_w"), 0] < row[0] and row[-1] < 1.0
    assert np.array_equal(vit.groups.layer_decay(cfg, 1.0), np.ones((20, L), F32))


def test_expand_dict_and_array(vit):
    cfg = vit.data.CONFIGS["test_h64"]
    names, L = vit.data.PARAM_NAMES, cfg.num_layers
    assert np.array_equal(vit.groups.expand(cfg, None), np.ones((20, L), F32))
    per_layer = [0.25, 1.5]
    t = vit.groups.expand(cfg, {"qkvw": per_layer, "head_b": 0.0, "fcb": 0.65, "wpe": 2})
    assert t.shape == (20, L) and t.dtype == F32
    want = np.ones((20, L), F32)
    want[names.index("qkvw")] = per_layer
    want[names.index("head_b")] = 0.0
    want[names.index("fcb")] = F32(0.65)
    want[names.index("wpe")] = 2.0
    assert np.array_equal(t, want)
    a = np.arange(20 * L, dtype=np.float64).reshape(20, L)
    got = vit.groups.expand(cfg, a)
    assert got.dtype == F32 and got.flags["C_CONTIGUOUS"] and np.array_equal(got, a.astype(F32))
    assert np.array_equal(vit.groups.expand(cfg, vit.groups.no_decay(cfg)), vit.groups.no_decay(cfg))


def test_expand_rejects_bad_input(vit):
    cfg = vit.data.CONFIGS["test_h64"]
    L = cfg.num_layers
    with pytest.raises(ValueError):
        vit.groups.expand(cfg, {"qkv_weight": 1.0})  # unknown name
    with pytest.raises(ValueError):
        vit.groups.expand(cfg, {"qkvw": [1.0] * (L + 1)})  # wrong length
    with pytest.raises(ValueError):
        vit.groups.expand(cfg, {"head_w": [1.0] * L})  # a per-layer list for a tensor outside the blocks
    with pytest.raises(ValueError):
        vit.groups.expand(cfg, np.ones((20, L + 1), F32))
    with pytest.raises(ValueError):
        vit.groups.expand(cfg, np.ones(20 * L, F32))
