"""bench.py --dump-outputs on the CPU: what dump_outputs writes for a step's outputs (float32 files under the size
budget, small arrays whole, large ones as the same seeded sample in every run) and the argument checks."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _outputs(seed):
    """the config-2 step's outputs by name, with a volume smaller than the real one but still over the budget"""
    g = torch.Generator().manual_seed(seed)
    n, h, w, d = 16, 432, 512, 40
    return [("lcn", torch.rand(n, 1, h, w, generator=g)), ("lcn_std", torch.rand(n, 1, h, w, generator=g)),
            ("disparity_index", torch.randint(0, 128, (n, h, w), generator=g)),
            ("best_score", torch.rand(n, h, w, generator=g)), ("cost_volume", torch.rand(n, d, h, w, generator=g)),
            ("geometric_loss", torch.tensor(0.25))]


def test_dump_outputs_budget_and_samples(tmp_path):
    b = _bench()
    outs = _outputs(0)
    m = b.dump_outputs(str(tmp_path / "a"), outs)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(n + ".npy" for n, _ in outs)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64e6
    for name, t in outs:
        a = np.load(tmp_path / "a" / (name + ".npy"))
        assert a.dtype == np.float32 and m[name]["shape"] == list(t.shape)
        if name == "cost_volume":
            assert m[name]["sampled"] and a.ndim == 1 and a.size >= b.DUMP_MIN_SAMPLE
            ix = np.sort(np.random.RandomState(b.DUMP_SEED).randint(0, t.numel(), size=a.size, dtype=np.int64))
            assert np.array_equal(a, t.reshape(-1).numpy()[ix])
        else:
            assert not m[name]["sampled"] and np.array_equal(a, t.float().numpy())   # indices exact in float32
    # the same outputs give the same files; different ones do not
    b.dump_outputs(str(tmp_path / "b"), _outputs(0))
    b.dump_outputs(str(tmp_path / "c"), _outputs(1))
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
    assert not np.array_equal(np.load(tmp_path / "a" / "cost_volume.npy"), np.load(tmp_path / "c" / "cost_volume.npy"))


def test_dump_outputs_float64_stays_float64(tmp_path):
    b = _bench()
    t = torch.arange(10, dtype=torch.float64) / 3
    b.dump_outputs(str(tmp_path), [("x", t), ("none", None)])
    assert os.listdir(tmp_path) == ["x.npy"]
    a = np.load(tmp_path / "x.npy")
    assert a.dtype == np.float64 and np.array_equal(a, t.numpy())


@pytest.mark.parametrize("flags", [["--steps", "0"], ["--warmup", "-1"]])
def test_step_counts_are_checked(monkeypatch, flags):
    b = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py"] + flags)
    with pytest.raises(SystemExit):
        b.parse_args()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "7", "--dump-outputs", "d"])
    a = b.parse_args()
    assert a.steps == 7 and a.dump_outputs == "d"
