"""bench.py --dump-outputs: what the last timed step computed is written as float .npy files, the parameter sample is the same
from run to run and stays inside the size bound, and the decoder's alias of the shared embedding is not counted twice.  Host
logic on a stand-in model: no GPU."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def _model(sd):
    return SimpleNamespace(hf_model=SimpleNamespace(engine=SimpleNamespace(state_dict=lambda: dict(sd))))


def test_small_model_is_dumped_whole_in_sorted_name_order(tmp_path):
    emb = torch.arange(6, dtype=torch.float32).reshape(2, 3)
    sd = {"b.weight": torch.tensor([7.0, 8.0]), "a.bias": torch.tensor([-1.0]), "embedding.w": emb, "decoder.embedding.w": emb}
    out = bench.last_step_outputs(_model(sd), [torch.tensor(2.5), torch.tensor(1.25)])
    assert out["losses"].dtype == np.float32 and out["losses"].tolist() == [2.5, 1.25]
    assert out["params"].dtype == np.float32 and out["params"].tolist() == [-1.0, 7.0, 8.0, 0.0, 1.0, 2.0, 3.0, 4.0, 5.0]
    bench.dump_outputs(out, str(tmp_path / "d"))
    assert sorted(os.listdir(tmp_path / "d")) == ["losses.npy", "params.npy"]
    assert np.array_equal(np.load(tmp_path / "d" / "params.npy"), out["params"])


def test_large_model_is_sampled_with_a_fixed_seed():
    g = torch.Generator().manual_seed(0)
    sd = {"w": torch.randn(5000, generator=g), "v": torch.randn(300, 7, generator=g)}
    a = bench.last_step_outputs(_model(sd), [torch.tensor(1.0)], sample=1000)["params"]
    b = bench.last_step_outputs(_model(sd), [torch.tensor(1.0)], sample=1000)["params"]
    assert a.shape == (1000,) and a.dtype == np.float32 and np.array_equal(a, b)
    full = torch.cat([sd["v"].reshape(-1), sd["w"]]).numpy()
    assert np.isin(a, full).all()
    # the default sample keeps the dump of any workload below 64 MB (the losses are a few bytes)
    assert bench.last_step_outputs.__defaults__[0] * 4 < 64 << 20
