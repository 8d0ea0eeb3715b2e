"""The plain bench run on the GPU (`bench.py --gpus 1 --steps K --warmup W`, no --full): it times
exactly K steps, prints one line with the contract's fields and nothing of the --full legs, and
--dump-outputs writes what the last timed step computed -- identical from run to run, and equal
to the oracle's results for the same seed."""
import json
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import oracle_ctypes as oc  # noqa: E402

SYSTEMS, LEN, SEED = 1000, 257, 0x5EED  # not a multiple of the wave or the workgroup


def _plain(out_dir, steps):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--systems", str(SYSTEMS), "--len", str(LEN), "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), {f.stem: np.load(f) for f in pathlib.Path(out_dir).glob("*.npy")}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump")
    return _plain(d / "a", 3), _plain(d / "b", 2)


def test_plain_line_has_the_contract_fields_and_no_full_legs(runs):
    (line, _), (line_b, _) = runs
    assert line["metric"].startswith("simulated instr/sec") and line["unit"] == "instr/s"
    assert line["higher_is_better"] is True and line["dtype"] == "u8" and line["n_gpus"] == 1
    assert line["steps"] == 3 and line_b["steps"] == 2 and line["warmup"] == 1
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(SYSTEMS * 8 * LEN / (line["ms_per_step"] / 1e3), rel=1e-3)
    assert 0 < line["kernel_ms_avg"] <= line["ms_per_step"] and line["roofline"]["bound"] == "hbm"
    assert line["totals"]["instructions_per_step"] == SYSTEMS * 8 * LEN
    assert line["full"] is False
    assert not {"contention", "sweep", "next", "cpu_baseline", "cpu_port", "box", "golden", "detail"} & set(line)


def test_dump_is_the_same_from_run_to_run(runs):
    (_, a), (_, b) = runs
    assert set(a) == set(b) == {"hist", "counters", "system_id", "digest_lo", "digest_hi", "rounds", "errors"}
    for k in a:
        assert a[k].dtype == np.float64 and np.array_equal(a[k], b[k]), k


def test_dump_equals_the_oracle(runs):
    (line, a), _ = runs
    ref = oc.run_batch(SEED, 0, SYSTEMS, num_procs=8, cache_size=4, length=LEN, threads=4)
    digests = (a["digest_hi"].astype(np.uint64) << np.uint64(32)) | a["digest_lo"].astype(np.uint64)
    assert a["system_id"].tolist() == list(range(SYSTEMS))
    assert np.array_equal(digests, ref["digests"]) and np.array_equal(a["rounds"], ref["rounds"])
    assert np.array_equal(a["errors"], ref["errors"])
    assert a["hist"].tolist() == ref["hist"].tolist() == line["totals"]["hist"]
    assert a["counters"][0] == SYSTEMS * 8 * LEN and a["counters"][3] == SYSTEMS
