"""CPU: bench.py --dump-outputs writes every tensor of a model output as <name>.npy in float32 / float64, within the byte
budget, large arrays as a fixed sample (same positions in every run)."""
import os

import numpy as np
import torch

import bench
from egtr_amd.egtr import DetrSceneGraphGenerationOutput


def _output(seed):
    g = torch.Generator().manual_seed(seed)
    return DetrSceneGraphGenerationOutput(
        logits=torch.randn(1, 200, 151, generator=g), pred_boxes=torch.rand(1, 200, 4, generator=g),
        pred_rel=torch.rand(1, 200, 200, 50, generator=g),
        decoder_hidden_states=tuple(torch.randn(1, 200, 256, generator=g) for _ in range(3)),
        encoder_hidden_states=tuple(torch.randn(1, 12537, 256, generator=g).to(torch.bfloat16) for _ in range(7)))


def test_output_arrays_flattens_nested_outputs():
    names = [n for n, _ in bench.output_arrays(_output(0))]
    assert names[:3] == ["logits", "pred_boxes", "pred_rel"]
    assert "decoder_hidden_states.2" in names and "encoder_hidden_states.6" in names
    loss = bench.output_arrays({"loss": torch.tensor(2.0), "loss_dict": {"a": 1.5, "b": torch.tensor(3)}})
    assert [n for n, _ in loss] == ["loss", "loss_dict.a", "loss_dict.b"]


def test_dump_outputs_budget_dtypes_and_fixed_samples(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 8_000_000)
    out = _output(0)
    arrays = bench.output_arrays(out) + [("index", torch.arange(10))]
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), arrays)
    bench.dump_outputs(str(b), arrays)
    files = sorted(os.listdir(a))
    assert files == sorted(n + ".npy" for n, _ in arrays)
    data = sum(np.load(a / f).nbytes for f in files)
    assert data <= 8_000_000
    for f in files:
        x, y = np.load(a / f), np.load(b / f)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y)
    assert np.load(a / "index.npy").dtype == np.float64
    logits = np.load(a / "logits.npy")                      # small: whole, in its shape
    assert logits.shape == (1, 200, 151) and np.array_equal(logits, out.logits.numpy())
    rel = np.load(a / "pred_rel.npy")                       # large: a 1-D sample of its elements
    assert rel.ndim == 1 and 0 < rel.size < out.pred_rel.numel()
    assert np.isin(rel, out.pred_rel.numpy().reshape(-1)).all()
