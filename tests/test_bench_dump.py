"""bench.py --dump-outputs without a GPU: the file layout, the 64 MB bound and the fixed row sample of large outputs."""
import os
import subprocess
import sys

import numpy as np

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_small_arrays_are_written_whole(tmp_path):
    terms = np.array([1.5, 2.5, 3.5])
    grad = np.arange(12, dtype=np.float32).reshape(3, 4)
    bench.dump_outputs(str(tmp_path / "out"), {"loss_terms": terms, "grad": grad})
    assert sorted(os.listdir(tmp_path / "out")) == ["grad.npy", "loss_terms.npy"]
    g = np.load(tmp_path / "out" / "grad.npy")
    assert g.dtype == np.float64 and np.array_equal(g, grad)
    assert np.array_equal(np.load(tmp_path / "out" / "loss_terms.npy"), terms)


def test_dump_outputs_samples_the_same_rows_under_the_bound(tmp_path):
    rng = np.random.default_rng(0)
    E = rng.standard_normal((4096, 1024))
    I = rng.standard_normal((4096, 1024))   # together 64 MiB: over the bound
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"ThryE": E, "ThryI": I})
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 64_000_000
    e, i = np.load(tmp_path / "a" / "ThryE.npy"), np.load(tmp_path / "a" / "ThryI.npy")
    assert e.shape[0] == i.shape[0] and e.shape[1] == 1024
    rows = [int(np.flatnonzero((E == r).all(axis=1))[0]) for r in e[:8]]
    assert rows == sorted(rows) and np.array_equal(i[:8], I[rows])   # ThryE and ThryI keep the same lineouts
    assert np.array_equal(e, np.load(tmp_path / "b" / "ThryE.npy"))   # fixed from run to run


def test_steps_must_be_positive():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "--steps must be at least 1" in p.stderr
