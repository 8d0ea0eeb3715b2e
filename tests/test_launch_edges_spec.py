"""The preconditions of tests/test_gpu_launch_edges.py, on the CPU: every cap the GPU tests cross is
still written where tests/launch_edges.py says it is, every shape crosses its cap, the tile and the
sources hold what the tests need, and the committed twin of the long shrink source
(tests/golden/shrink_long.json) is what tests/shrink_ref.py says it is. No device call is made here."""
import numpy as np
import pytest

import launch_edges as le
import oracle_ctypes as oc
import shrink_ref as sr
from test_gpu_tiers import contended, contended_oracle, depth_of


@pytest.mark.parametrize("name", sorted(le.CAP_SOURCES))
def test_caps_are_written_where_the_helper_says(name):
    text = (le.CSRC / name).read_text()
    for line in le.CAP_SOURCES[name]:
        assert line in text, f"{name} no longer holds: {line}"


def test_large_shape_crosses_every_grid_stride_loop():
    assert le.nchunks(le.MAX_INSTR) == le.nchunks(le.MAXLEN) == 16 and le.ROW == 128
    groups = le.S // (64 // le.N)
    assert le.S % (64 // le.N) == 0 and groups * le.nchunks(le.MAX_INSTR) * 64 == le.S * le.ROW == 5_120_000
    assert le.S * le.ROW > le.GRID_STRIDE_THREADS == 4_194_304
    # the second trip of a 4M-thread loop over chunks starts at this system
    assert le.GRID_STRIDE_THREADS % le.ROW == 0 and le.GRID_STRIDE_THREADS // le.ROW == 32_768 < le.S - le.T
    # coherence: more workgroups of work than MAX_TRIPS, so a grid of one is raised to two
    blocks = -(-groups // le.COH_WAVES)
    assert blocks == 1250 > le.COH_MAX_TRIPS and -(-blocks // le.COH_MAX_TRIPS) == 2
    # the event log: [sys][round / 4][node][round % 4] words; byte 2^32 is the first of system 32,768
    per_sys = le.N * le.EVENT_ROUNDS * 4
    assert le.EVENT_ROUNDS % 4 == 0 and le.S * per_sys == 5_242_880_000 and (1 << 32) // per_sys == 32_768
    assert (1 << 32) % per_sys == 0


def test_tile_holds_what_the_tests_need():
    packed, lens = le.tile()
    assert packed.shape == (le.T, le.N, le.MAXLEN) and not lens[0].any() and lens.max() == le.MAXLEN
    for seed in (0, le.TILE_RNG):
        runs, recs = le.tile_runs(seed), le.tile_coherence(seed)
        bits = [r["bits"] for r in recs]
        assert 0 < sum(b != 0 for b in bits) < le.T  # clean and violating systems
        assert bin(int(np.bitwise_or.reduce(bits))).count("1") >= 6
        assert recs[0] == {"bits": 0, "addrs": 0, "first_addr": 0xFFFFFFFF, "first_bits": 0}
        assert max(res.rounds for res, _ in runs) <= le.EVENT_ROUNDS  # the log holds every run
        assert {res.rounds % 4 for res, _ in runs} == {0, 1, 2, 3}
        assert len({res.digest for res, _ in runs}) > le.T // 2  # a tile of distinct systems
    # the tile is no period of a wave: entry j meets every lane position
    assert all(len({(j + m * le.T) % (64 // le.N) for m in range(64 // le.N)}) == 64 // le.N for j in (0, 1, 96))


def test_rd_rule_in_numpy():
    packed = np.array([[[0x8134, 0x0134, 0x0100, 0x9200]]], np.uint16)
    lens = np.array([[3]], np.uint32)
    assert le.clear_rd(packed, lens).tolist() == [[[0x8134, 0x0100, 0x0100, 0]]]
    dirty = le.with_rd_garbage(packed, np.random.default_rng(0))
    assert (dirty[0, 0, [0, 3]] == packed[0, 0, [0, 3]]).all() and (dirty[0, 0, 1:3] & 0xFF).all()
    assert np.array_equal(le.clear_rd(dirty, lens), le.clear_rd(packed, lens))


def test_explore_shapes(dash):
    # explore(src, 0, 40,500) on S systems: two passes, the last one padded
    assert le.S < 40_500 < 2 * le.S
    # explore_sources: R rows per source, two passes, 24 fresh rows in the second, 12 padding systems
    G, K = le.SRC_G, le.SRC_K
    R = le.S // G
    assert (R, -(-K // R), K - R, le.S - G * R) == (3076, 2, 24, 12)
    assert le.S * le.ROW > le.GRID_STRIDE_THREADS  # replicate's second trip
    assert 64 <= 2 * G * K <= 131_072 < 4 * G * K  # the default table: next_pow2(2 * schedules) slots
    # dash_explore_assign agrees: the last system of the last source is counted in pass 0 only, and the
    # 12 systems past G * R never are
    assert dash.explore_assign(le.S, G, K, 0, 0, G * R - 1)[2]
    assert not dash.explore_assign(le.S, G, K, 0, 1, G * R - 1)[2]
    assert dash.explore_assign(le.S, G, K, 0, 1, G * 23 + 5)[2]
    assert not any(dash.explore_assign(le.S, G, K, 0, p, k)[2] for p in (0, 1) for k in range(G * R, le.S))
    packed, lens = le.racy_sources()
    assert packed.shape == (G, le.N, le.SRC_LEN)
    for s in range(G):
        seen = {(r.digest, r.errors) for r in (oc.run_system(packed[s], lens[s], num_procs=le.N, cache_size=le.CS,
                                                             arb_seed=seed) for seed in range(le.SRC_PROBE))}
        assert len(seen) > 1, s


def test_shrink_y_stride_shape():
    row = sr.ROWS[1]
    assert row[3] == 0  # a lockstep row
    assert le.SHRINK_Y_SYSTEMS > le.VARIANT_MAX_Y  # the last system is written by the y-stride only
    assert le.SHRINK_Y_SYSTEMS - 1 >= le.VARIANT_MAX_Y


def replay(lens, steps):
    """The lengths before every step, and after the last."""
    ln = [int(x) for x in lens]
    out = []
    for t, _s, n, _c in steps:
        out.append(list(ln))
        ln[t] -= n
    return out, ln


def test_shrink_long_fixture():
    """The committed twin, re-checked without the twin's search: the source meets the goal, every
    step's winner passes on the base of its round and has that base's candidate count, and the
    final set is 1-minimal (no single candidate of it passes)."""
    rec = le.long_fixture()
    k, tr, lens, bits = le.long_source(rec["rng"])
    goal = (rec["bit"], 0, 0xFFFFFFFF)
    assert k == rec["index"] and rec["bit"] == bits & -bits and lens.tolist() == [le.LONG_M] * le.LONG_N
    N, CS = le.LONG_N, le.LONG_CS
    assert sr.passes(*sr.outcome(tr, lens, N, CS, 0), goal)
    twin_tr, twin_ln, steps = rec["twin"]
    cur_tr, cur_ln = tr.copy(), lens.copy()
    for t, s, n, C in steps:
        cands = sr.candidates(cur_ln)
        assert len(cands) == C and (t, s, n) in cands
        cur_tr, cur_ln = sr.delete(cur_tr, cur_ln, t, s, n)
        assert sr.passes(*sr.outcome(cur_tr, cur_ln, N, CS, 0), goal), (t, s, n)
    assert cur_ln.tolist() == twin_ln.tolist() and np.array_equal(cur_tr[:, :twin_tr.shape[1]], twin_tr)
    assert not cur_tr[:, twin_tr.shape[1]:].any()
    for t, s, n in sr.candidates(cur_ln):
        assert not sr.passes(*sr.outcome(*sr.delete(cur_tr, cur_ln, t, s, n), N, CS, 0), goal), (t, s, n)
    # what the GPU test needs of it: 152 chunks per stream, 1,216 items, two x-blocks; three sub-passes
    # in the first round; a winner on node 6 or 7 while the launch still has two x-blocks
    W = le.write_chunks(le.LONG_M, le.LONG_M)
    assert (W, N * W, -(-N * W // le.VARIANT_ITEMS_PER_BLOCK)) == (152, 1216, 2)
    assert steps[0][3] == 9624 and -(-steps[0][3] // le.LONG_S) == 3
    before, _ = replay(lens, steps)
    assert any(t >= 6 and N * le.write_chunks(le.LONG_M, max(b)) > le.VARIANT_ITEMS_PER_BLOCK
               for (t, _s, _n, _c), b in zip(steps, before))


def test_directory_slabs():
    assert le.text_slot(le.DIR_M) == 77_824 and le.per_slab(le.DIR_M, le.N, le.DIR_ENTRIES) == 107
    p = le.per_slab(le.DIR_M, le.N, le.DIR_ENTRIES)
    assert [min(p, le.DIR_ENTRIES - s0) for s0 in range(0, le.DIR_ENTRIES, p)] == [107, 107, 36]  # slab 0 reused
    packed, lens = le.dir_traces()
    assert lens[0, 3] == le.DIR_M and lens[1, 5] == 0
    order = le.dir_order()
    assert len(order) == le.DIR_ENTRIES and set(order.tolist()) == set(range(le.DIR_DISTINCT))
    assert {0, 1} <= set(order[:p].tolist()) and {0, 1} <= set(order[2 * p:].tolist())  # in the first slab and the last


def test_mark_source_is_deeper_than_32():
    assert le.MARK_SYSTEMS > le.MARK_THREADS == 262_144
    depth = depth_of(contended_oracle(8, 1, 200, 0))
    s = int(np.argmax(depth))
    assert depth[s] > 32 and contended(8, 1, 200)[1][s].tolist() == [200] * 8


def test_digest_windows():
    n = le.DIGEST_SYSTEMS
    window = 2 * le.DIGEST_THREADS * le.DIGEST_CHUNK
    assert n == 2_167_152 and window < n < 2 * window and (n - window) % le.DIGEST_CHUNK != 0
    assert (n - window) // le.DIGEST_CHUNK >= 1  # the second window has a second chunk too

