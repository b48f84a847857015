"""The checkpoint format against an independent numpy statement of it (tests/ckpt_format.py: the header slots
[0..26] and the section order of include/vit_checkpoint.h), for all eight layouts (AdamW state x EMA x momentum
buffer): the writer's bytes, the four readers' results, corrupt sizes and a config mismatch; and the stand-alone
host program tests/host/checkpoint_roundtrip.cpp.  Every comparison is on bits.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ckpt_format

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
HP = (0.9, 0.95, 1e-8, 0.1)
SGD = (0.9, 0.0, 5e-4, True)
STEP, DECAY = 7, 0.9999
UPDATES, MSTEPS = (1 << 33) + 5, (1 << 34) + 3  # both halves of each 64-bit count


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def cfg(vit):
    return vit.data.CONFIGS["test"]


@pytest.fixture(scope="module")
def arrs(cfg):
    rng = np.random.default_rng(26)
    p, m, v, e, b = (rng.standard_normal(cfg.num_params()).astype(F32) for _ in range(5))
    p[:3] = [-0.0, np.inf, 1e-45]  # bits a value comparison would not tell apart or would refuse
    return p, m, np.abs(v), e, b


def kwargs(arrs, opt, ema, mom):
    """the arguments of vit.write_checkpoint and ckpt_format.encode for one layout"""
    p, m, v, e, b = arrs
    kw = dict(params=p)
    if opt:
        kw.update(m=m, v=v, step=STEP, adamw=HP)
    if ema:
        kw.update(ema=e, ema_decay=DECAY, ema_updates=UPDATES)
    if mom:
        kw.update(momentum=b, sgd=SGD, momentum_steps=MSTEPS)
    return kw


@pytest.mark.parametrize("opt,ema,mom", ckpt_format.LAYOUTS)
def test_writer_bytes(vit, cfg, arrs, tmp_path, opt, ema, mom):
    """(a) write_checkpoint's file is the numpy statement's, byte for byte"""
    kw = kwargs(arrs, opt, ema, mom)
    path = tmp_path / "w.bin"
    vit.write_checkpoint(path, cfg, **kw)
    assert path.read_bytes() == ckpt_format.encode(cfg, **kw)
    assert not os.path.exists(str(path) + ".tmp")
    # the arguments of an absent section are ignored: the same bytes with every scalar passed anyway
    vit.write_checkpoint(path, cfg, **{**dict(step=STEP, adamw=HP, ema_decay=DECAY, ema_updates=UPDATES, sgd=SGD,
                                               momentum_steps=MSTEPS), **kw})
    assert path.read_bytes() == ckpt_format.encode(cfg, **kw)


@pytest.mark.parametrize("opt,ema,mom", ckpt_format.LAYOUTS)
def test_reader_results(vit, cfg, arrs, tmp_path, opt, ema, mom):
    """(b) a file the numpy statement wrote comes back through the four readers: arrays on bits, every scalar"""
    p, m, v, e, b = arrs
    path = tmp_path / "r.bin"
    path.write_bytes(ckpt_format.encode(cfg, **kwargs(arrs, opt, ema, mom)))
    info = vit.checkpoint_info(path)
    c = info["cfg"]
    assert (c.img, c.patch, c.channels, c.num_layers, c.num_heads, c.num_classes, c.in_ch) == (
        cfg.img, cfg.patch, cfg.channels, cfg.num_layers, cfg.num_heads, cfg.num_classes, cfg.in_ch)
    assert info["num_params"] == cfg.num_params() and info["has_opt"] is opt
    assert info["step"] == (STEP if opt else 0)
    assert info["adamw"] == (tuple(float(F32(x)) for x in HP) if opt else (0.0, 0.0, 0.0, 0.0))
    p2, m2, v2 = vit.read_checkpoint(path, cfg)
    assert np.array_equal(bits(p2), bits(p))
    if opt:
        assert np.array_equal(bits(m2), bits(m)) and np.array_equal(bits(v2), bits(v))
    else:
        assert m2 is None and v2 is None
    e2, d2, u2 = vit.read_checkpoint_ema(path, cfg)
    if ema:
        assert np.array_equal(bits(e2), bits(e)) and (d2, u2) == (float(F32(DECAY)), UPDATES)
    else:
        assert (e2, d2, u2) == (None, 0.0, 0)
    b2, sg, st = vit.read_checkpoint_momentum(path, cfg)
    if mom:
        assert np.array_equal(bits(b2), bits(b)) and st == MSTEPS
        assert sg == (float(F32(SGD[0])), float(F32(SGD[1])), float(F32(SGD[2])), True)
    else:
        assert (b2, sg, st) == (None, (0.0, 0.0, 0.0, False), 0)


def readers(vit, cfg):
    return [lambda path: vit.checkpoint_info(path), lambda path: vit.read_checkpoint(path, cfg),
            lambda path: vit.read_checkpoint_ema(path, cfg), lambda path: vit.read_checkpoint_momentum(path, cfg)]


@pytest.mark.parametrize("opt,ema,mom", ckpt_format.LAYOUTS)
def test_corrupt_sizes_are_refused(vit, cfg, arrs, tmp_path, opt, ema, mom):
    """(c) 4 bytes short and 4 bytes long: every reader refuses both"""
    raw = ckpt_format.encode(cfg, **kwargs(arrs, opt, ema, mom))
    path = tmp_path / "c.bin"
    for cut in (raw[:-4], raw + b"\0\0\0\0"):
        path.write_bytes(cut)
        for read in readers(vit, cfg):
            with pytest.raises(vit.VitError):
                read(path)


@pytest.mark.parametrize("opt,ema,mom", ckpt_format.LAYOUTS)
def test_config_mismatch_is_refused(vit, cfg, arrs, tmp_path, opt, ema, mom):
    """(d) the three array readers refuse a file of another config (the header reader has none to compare)"""
    path = tmp_path / "d.bin"
    path.write_bytes(ckpt_format.encode(cfg, **kwargs(arrs, opt, ema, mom)))
    other = vit.data.CONFIGS["test_h64"]
    for read in readers(vit, other)[1:]:
        with pytest.raises(vit.VitError, match="config differs"):
            read(path)
    assert vit.checkpoint_info(path)["num_params"] == cfg.num_params()


def test_host_roundtrip_program(tmp_path):
    """tests/host/checkpoint_roundtrip.cpp linked with csrc/checkpoint.cpp alone, by the host compiler of
    vit.rs_amd/Makefile ($(CXX), make's default g++): every layout through every public reader with every
    combination of NULL out pointers, and every cut file refused with the caller's buffers untouched"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "checkpoint_roundtrip"
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "host", "checkpoint_roundtrip.cpp"),
                    os.path.join(ROOT, "vit.rs_amd", "csrc", "checkpoint.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "checkpoint_roundtrip ok: 8 layouts" in out.stdout
