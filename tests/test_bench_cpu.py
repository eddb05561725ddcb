"""bench.py's --dump-outputs writer on the CPU: the whole vector when it is small, otherwise a fixed seeded sample of it with its
positions; the same sample from run to run."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")


def test_dump_outputs_whole_vector_and_seeded_sample(tmp_path, monkeypatch):
    import bench
    Y = torch.linspace(-1.0, 2.0, 3000, dtype=torch.float64).reshape(1, -1)
    bench.dump_outputs(str(tmp_path / "whole"), Y)
    assert sorted(p.name for p in (tmp_path / "whole").iterdir()) == ["y.npy", "y_norms.npy"]
    assert np.array_equal(np.load(tmp_path / "whole" / "y.npy"), Y.numpy().reshape(-1))

    monkeypatch.setattr(bench, "DUMP_MAX_ENTRIES", 500)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), Y)
    names = ["y_norms.npy", "y_sample.npy", "y_sample_index.npy"]
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == names
    for name in names:
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype == np.float64 and np.array_equal(a, b)
    idx = np.load(tmp_path / "a" / "y_sample_index.npy")
    assert 0 < idx.size <= 500 and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 3000
    assert np.array_equal(np.load(tmp_path / "a" / "y_sample.npy"), Y.numpy().reshape(-1)[idx.astype(np.int64)])
    y = Y.numpy().reshape(-1)
    assert np.allclose(np.load(tmp_path / "a" / "y_norms.npy"), [np.linalg.norm(y), y.sum(), np.abs(y).max()], rtol=1e-12)
