"""bench.py's command line and --dump-outputs writer (no GPU): a plain run is
the headline only, --full / --extras switch the rest on, and a dump is float32
/ float64 .npy files of at most 64 MB — a large embedding table is cut to the
same seeded sample of rows every time."""
import os
import types

import numpy as np
import torch

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr("sys.argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_headline_only(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.extras, a.dump_outputs) == (7, 2, False, False, None)
    assert _parse(monkeypatch, "--full").full
    assert _parse(monkeypatch, "--extras").full  # the other paths are part of the full report
    assert _parse(monkeypatch, "--dump-outputs", "d").dump_outputs == "d"


def _map(n_rows):
    emb = torch.arange(n_rows, dtype=torch.float32).reshape(-1, 1).repeat(1, 16)
    dec = torch.nn.Sequential(torch.nn.Linear(16, 8), torch.nn.Linear(8, 4))
    kfs = [types.SimpleNamespace(pose=types.SimpleNamespace(data=torch.full((6,), float(f)))) for f in range(3)]
    return emb, dec, kfs


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_small(tmp_path):
    emb, dec, kfs = _map(1000)
    bench.dump_outputs(str(tmp_path / "d"), emb, dec, kfs)
    got = _load(tmp_path / "d")
    assert sorted(got) == ["decoder.0.bias", "decoder.0.weight", "decoder.1.bias", "decoder.1.weight",
                           "embeddings", "poses"]
    assert all(a.dtype == np.float32 for a in got.values())
    assert np.array_equal(got["embeddings"], emb.numpy())
    assert np.array_equal(got["decoder.1.weight"], dec[1].weight.detach().numpy())
    assert np.array_equal(got["poses"], np.repeat(np.arange(3, dtype=np.float32)[:, None], 6, 1))


def test_dump_outputs_large_table_is_a_seeded_sample(tmp_path):
    n = (48 << 20) // 64 + 1000  # just past the table's share of the 64 MB
    emb, dec, kfs = _map(n)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), emb, dec, kfs)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    rows = a["embeddings_rows"]
    assert rows.dtype == np.float64 and np.array_equal(rows, b["embeddings_rows"])
    assert len(rows) == (48 << 20) // 64 and np.all(np.diff(rows) > 0) and rows[-1] < n
    assert a["embeddings"].dtype == np.float32
    assert np.array_equal(a["embeddings"][:, 0], rows.astype(np.float32))  # row r holds the value r
