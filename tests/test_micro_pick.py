"""dash_micro_pick, the seeded micro-step schedule's rule (include/dash.h), and the committed
witnesses of tests/golden/schedules/micro_seeds.json (CPU only).

The witnesses are checked in the oracle's STRICT model through the twin walk (tests/micro_twin.py):
each (weights, seed) must walk, step by step accepted, to a terminal state of the recorded length
whose dumps are the reference's accepted run_k files.
"""
import json
import math

import numpy as np
import pytest

import micro_twin
import oracle_ctypes as oc
from oracle_ctypes import GOLDEN

RECORDS = json.loads((GOLDEN.parent / "schedules" / "micro_seeds.json").read_text())["records"]
SEEDS = [87, 0xABCDEF, (1 << 64) - 1, 0x5EED5EED12345678]


def test_pick_is_enabled_and_lone_node_is_picked(dash):
    rng = np.random.default_rng(77)
    for N in (1, 2, 3, 4, 8):
        for t in range(N):  # a lone enabled node, whatever its weight
            for w in (0, 1, 31):
                weights = [int(x) for x in rng.integers(0, 32, size=N)]
                weights[t] = w
                assert dash.micro_pick(int(rng.integers(0, 1 << 63)), int(rng.integers(0, 1 << 31)), 1 << t,
                                       weights, N) == t
        for _ in range(2000):
            en = int(rng.integers(1, 1 << N))
            weights = [int(x) for x in rng.integers(0, 32, size=N) * rng.integers(0, 2, size=N)]
            t = dash.micro_pick(int(rng.integers(0, 1 << 63)), int(rng.integers(0, 1 << 32)), en, weights, N)
            assert 0 <= t < N and (en >> t) & 1
            if any(weights[k] for k in range(N) if (en >> k) & 1):  # a weight-0 node only when all are
                assert weights[t] > 0


def test_weight_zero_nodes_are_picked_uniformly_among_themselves(dash):
    """Enabled nodes 1, 2, 5 of 8 all have weight 0 (node 0, weight 31, is not enabled): each is
    picked, within 6 binomial standard deviations of a third of the rounds."""
    R = 30000
    cnt = [0] * 8
    for r in range(R):
        cnt[dash.micro_pick(413, r, 0b100110, [31, 0, 0, 7, 7, 0, 7, 7], 8)] += 1
    sd = math.sqrt(R * (1 / 3) * (2 / 3))
    assert sum(cnt[k] for k in (1, 2, 5)) == R
    assert all(abs(cnt[k] - R / 3) <= 6 * sd for k in (1, 2, 5)), cnt


def test_argument_errors(dash):
    L = dash.lib()
    U = dash.MICRO_UNIFORM
    assert L.dash_micro_pick(1, 0, 0, U, 4) == dash.EINVAL           # nothing enabled
    assert L.dash_micro_pick(1, 0, 0b10000, U, 4) == dash.EINVAL     # a bit >= num_procs
    assert L.dash_micro_pick(1, 0, 1 << 8, U, 8) == dash.EINVAL
    assert L.dash_micro_pick(1, 0, 1, 32, 4) == dash.EINVAL          # a weight byte > 31
    assert L.dash_micro_pick(1, 0, 1, 0xFF << 56, 4) == dash.EINVAL  # also of a node past num_procs
    assert L.dash_micro_pick(1, 0, 1, U, 0) == dash.EINVAL
    assert L.dash_micro_pick(1, 0, 1, U, 9) == dash.EINVAL
    assert L.dash_micro_pick(1, 0, 0b1111, 31 * U, 4) in range(4)


def test_pick_is_the_stated_formula(dash):
    """Restated in Python: u = high 32 bits of fmix64(seed ^ round * golden), x = (u * W) >> 32, the
    lowest enabled node whose inclusive enabled weight sum exceeds x."""
    rng = np.random.default_rng(5)
    M = (1 << 64) - 1
    for _ in range(3000):
        N = int(rng.integers(1, 9))
        en = int(rng.integers(1, 1 << N))
        w = [int(x) for x in rng.integers(0, 32, size=N) * rng.integers(0, 2, size=N)]
        seed, rnd = int(rng.integers(0, 1 << 63)) * 2 + 1, int(rng.integers(0, 1 << 32))
        ws = [w[t] if (en >> t) & 1 else 0 for t in range(N)]
        if sum(ws) == 0:
            ws = [(en >> t) & 1 for t in range(N)]
        x = ((oc._fmix(seed ^ ((rnd * 0x9E3779B97F4A7C15) & M)) >> 32) * sum(ws)) >> 32
        acc, want = 0, None
        for t in range(N):
            acc += ws[t]
            if acc > x:
                want = t
                break
        assert dash.micro_pick(seed, rnd, en, w, N) == want


def test_frequencies_follow_the_weights(dash):
    """Rounds 0..65,535 of four seeds, all of 4 nodes enabled, weights (1, 2, 4, 8): each node's
    count within 6 binomial standard deviations of 65536 * w / 15."""
    R, w = 65536, (1, 2, 4, 8)
    L, packed = dash.lib(), dash.pack_weights(w)
    for seed in SEEDS:
        cnt = np.bincount([L.dash_micro_pick(seed, r, 0b1111, packed, 4) for r in range(R)], minlength=4)
        for t in range(4):
            p = w[t] / 15
            assert abs(int(cnt[t]) - R * p) <= 6 * math.sqrt(R * p * (1 - p)), (hex(seed), cnt.tolist())


def test_records_cover_the_accepted_runs():
    assert sorted((r["test"], r["run"]) for r in RECORDS) == \
        [("test_3", "run_1"), ("test_3", "run_2")] + [("test_4", f"run_{k}") for k in (1, 2, 3, 4)]


@pytest.mark.parametrize("rec", RECORDS, ids=lambda r: f"{r['test']}-{r['run']}")
def test_witness_walks_to_the_accepted_run(dash, rec):
    tr, lens = oc.load_test_dir(GOLDEN / rec["test"])
    # every step of the walk was accepted by STRICT (the twin only appends accepted steps, and the
    # final replay of the whole witness raises on one that is not)
    steps, out, term = micro_twin.walk(tr, lens, rec["seed"], rec["weights"], 4, 4)
    assert term and out.errors == 0
    assert len(steps) == rec["rounds"]
    assert out.digest == int(rec["digest"], 16)
    for n in range(4):
        assert oc.dump_node(out, n).encode() == (GOLDEN / rec["test"] / rec["run"] / f"core_{n}_output.txt").read_bytes()
