"""bench.py's command line and output dump, as far as they run without a GPU: a plain run is the headline only
(--full is off by default), and --dump-outputs writes float arrays of a bounded size that depend only on the step's
outputs (the column sample is fixed)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_headline_only(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 2)
    assert a.full is False and a.dump_outputs is None
    a = _parse(monkeypatch, "--full", "--dump-outputs", "somewhere")
    assert a.full is True and a.dump_outputs == "somewhere"


def test_dump_outputs_writes_bounded_float_arrays_with_a_fixed_sample(tmp_path):
    vocab, rows = 128256, 3                     # the benchmark's vocabulary; the rows do not enter the sampling
    g = torch.Generator().manual_seed(1)
    logits = torch.randn(rows, vocab, generator=g).to(torch.bfloat16)
    ids = torch.argmax(logits, dim=-1)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), logits, ids)
    got = {n: np.load(tmp_path / "a" / n) for n in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(got) == ["logits_sample.npy", "logits_sample_columns.npy", "next_token_ids.npy"]
    for n, arr in got.items():
        assert arr.dtype in (np.float32, np.float64)
        assert np.array_equal(arr, np.load(tmp_path / "b" / n))          # same arguments, same files
    cols = got["logits_sample_columns.npy"].astype(np.int64)
    assert cols.shape == (bench.DUMP_LOGIT_COLUMNS,) and len(set(cols.tolist())) == len(cols)
    assert cols.min() >= 0 and cols.max() < vocab and np.all(np.diff(cols) > 0)
    assert np.array_equal(got["logits_sample.npy"], logits.float().numpy()[:, cols])
    assert np.array_equal(got["next_token_ids.npy"], ids.numpy().astype(np.float64))
    # at the benchmark's largest batch (256 rows) the three files stay far below 64 MB
    assert 256 * bench.DUMP_LOGIT_COLUMNS * 4 + bench.DUMP_LOGIT_COLUMNS * 8 + 256 * 8 < 64 * 10 ** 6
