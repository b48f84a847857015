"""CPU checks of bench.py's command line: --full / --dump-outputs exist and default off, and
dump_outputs writes float arrays of bounded total size at a sample that is the same every run."""
import os
import sys
import types

import numpy as np

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_plain_run_is_the_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"


class _FakeModel:
    h = None
    B, NC = 4, 10

    def __init__(self, n):
        self.num_parameters = n

    def logits(self):
        return np.arange(self.B * self.NC, dtype=np.float32).reshape(self.B, self.NC)

    def grads(self):
        return np.arange(self.num_parameters, dtype=np.float32)

    def params(self):
        return -np.arange(self.num_parameters, dtype=np.float32)


def _fake_vit():
    lib = types.SimpleNamespace(vit_trainer_mean_loss=lambda h: 1.5)
    return types.SimpleNamespace(lib=lambda: lib, check=lambda what="": None)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_small_model_keeps_everything(monkeypatch, tmp_path):
    monkeypatch.setattr(bench, "vit", _fake_vit())
    m = _FakeModel(1000)
    bench.dump_outputs(m, str(tmp_path / "a"))
    out = _load(tmp_path / "a")
    assert set(out) == {"loss", "logits", "grads", "params", "sample_index"}
    assert all(v.dtype in (np.float32, np.float64) for v in out.values())
    assert out["loss"].tolist() == [1.5]
    np.testing.assert_array_equal(out["grads"], m.grads())
    np.testing.assert_array_equal(out["params"], m.params())
    np.testing.assert_array_equal(out["logits"], m.logits())


def test_dump_outputs_large_model_is_a_fixed_bounded_sample(monkeypatch, tmp_path):
    monkeypatch.setattr(bench, "vit", _fake_vit())
    m = _FakeModel(3 * bench.DUMP_SAMPLE + 7)
    bench.dump_outputs(m, str(tmp_path / "a"))
    bench.dump_outputs(m, str(tmp_path / "b"))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(v.nbytes for v in a.values()) <= 64 * 1000 * 1000
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    idx = a["sample_index"].astype(np.int64)
    assert idx.size == bench.DUMP_SAMPLE and idx.min() >= 0 and idx.max() < m.num_parameters
    assert np.all(np.diff(idx) >= 0)
    np.testing.assert_array_equal(a["grads"], m.grads()[idx])
    np.testing.assert_array_equal(a["params"], m.params()[idx])
