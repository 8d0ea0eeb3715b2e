"""bench.py --dump-outputs (CPU only): the files a run leaves are the float64 images of what
dash_run returned and dash_read_results holds; an output above the size limit becomes a fixed,
seeded sample of the systems that is the same in every run."""
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402

NAMES = {"hist", "counters", "system_id", "digest_lo", "digest_hi", "rounds", "errors"}


class FakeEngine:
    """read_results() of n systems with digests that use all 64 bits."""

    def __init__(self, n, seed=7):
        rng = np.random.default_rng(seed)
        self.d = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
        self.d[0] = np.uint64(0xFFFFFFFFFFFFFFFF)
        self.r = rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
        self.e = rng.integers(0, 64, size=n, dtype=np.uint32)

    def read_results(self):
        return self.d, self.r, self.e


STATS = {"hist": list(range(100, 113)), "instructions": 1 << 35, "rounds_total": 12345678901, "rounds_max": 99,
         "systems": 1000, "err_systems": 5, "err_bits": 6, "dropped": 7, "max_depth": 16, "kernel_ms": 1.5,
         "tier_systems": [1000, 0, 0], "wave_rounds": 1}


def _load(d, suffix=""):
    return {f.name[:-len(suffix + ".npy")]: np.load(f) for f in pathlib.Path(d).glob(f"*{suffix}.npy")}


def test_dump_is_exact_and_complete(tmp_path):
    eng = FakeEngine(1000)
    bench.dump_outputs(eng, STATS, tmp_path / "out")
    got = _load(tmp_path / "out")
    assert set(got) == NAMES and all(a.dtype == np.float64 for a in got.values())
    assert got["hist"].tolist() == STATS["hist"]
    assert got["counters"].tolist() == [1 << 35, 12345678901, 99, 1000, 5, 6, 7, 16]
    assert got["system_id"].tolist() == list(range(1000))
    # the two 32-bit halves are exact in float64 and give the digest back
    back = (got["digest_hi"].astype(np.uint64) << np.uint64(32)) | got["digest_lo"].astype(np.uint64)
    assert np.array_equal(back, eng.d)
    assert np.array_equal(got["rounds"], eng.r) and np.array_equal(got["errors"], eng.e)


def test_large_output_is_a_fixed_sample_within_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT", 64 << 10)
    eng = FakeEngine(5000)
    bench.dump_outputs(eng, STATS, tmp_path / "a")
    bench.dump_outputs(eng, STATS, tmp_path / "b")
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 64 << 10
    ids = a["system_id"].astype(np.int64)
    assert 1000 < len(ids) < 5000 and np.all(np.diff(ids) > 0) and ids[-1] < 5000
    assert all(np.array_equal(a[k], b[k]) for k in NAMES)  # the same systems in every run
    assert np.array_equal(a["rounds"], eng.r[ids]) and np.array_equal(a["errors"], eng.e[ids])
    assert np.array_equal(a["digest_lo"], (eng.d[ids] & np.uint64(0xFFFFFFFF)).astype(np.float64))


def test_other_ranks_write_beside_rank_zero(tmp_path):
    bench.dump_outputs(FakeEngine(10), STATS, tmp_path, rank=0)
    bench.dump_outputs(FakeEngine(10, seed=8), STATS, tmp_path, rank=3)
    assert set(_load(tmp_path, ".rank3")) == NAMES
    assert len(list(tmp_path.glob("*.npy"))) == 2 * len(NAMES)
