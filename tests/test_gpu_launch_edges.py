"""The kernels around sim_kernel where a launch takes a second trip, block or slab: the grid-stride
loops of clear_rd, broadcast, replicate and mark past their capped grids, many_variant_kernel's y-stride
and second x-block, coherence_kernel's walk of several trips and its grid floor, the event log past
byte 2^32, dash_load_dirs_device's reuse of a pinned slab, and dash_write_digests' second window.

Each test takes its path across the boundary at the smallest handle that crosses it (the shapes and
the caps they cross: tests/launch_edges.py, kept true on the CPU by tests/test_launch_edges_spec.py)
and compares with a reference that stays small. The large batches repeat a tile of T = 97 systems:
runs are deterministic, so every per-system result must equal that of its tile entry (one numpy
comparison over the batch), the first T systems are checked against the existing references -- the
oracle, tests/coherence_ref.py, tests/metrics_ref.py -- and totals against sums over the records."""
import os

import numpy as np
import pytest

import coherence_ref as cr
import launch_edges as le
import metrics_ref as mr
import oracle_ctypes as oc
import shrink_ref as sr
from test_gpu_explore_sources import OUT_FIELDS, check_sums
from test_gpu_metrics import as_dicts, check_totals, events_of
from test_gpu_shrink import check_against_twin, engine as shrink_engine, load_batch as load_shrink_batch
from test_gpu_tiers import contended, contended_oracle, depth_of, tier_counts

pytestmark = pytest.mark.gpu
S, T, N, CS = le.S, le.T, le.N, le.CS
FAR = (32_767, 32_768, 32_769, S - 1)  # around the second trip's first system, and the last


def big_engine(dash, **kw):
    return dash.Engine(S, num_procs=N, cache_size=CS, max_instr=le.MAX_INSTR, **kw)


def load_tiled(eng):
    packed, lens = le.tile()
    eng.load_traces(le.tiled(packed), le.tiled(lens))


def check_results_tiled(eng, stats, seed=0):
    """Digests, rounds and errors of the whole batch equal their tile entries', and those the oracle's."""
    dig, rnd, err = eng.read_results()
    runs = le.tile_runs(seed)
    assert dig[:T].tolist() == [res.digest for res, _ in runs]
    assert rnd[:T].tolist() == [res.rounds for res, _ in runs]
    assert err[:T].tolist() == [res.errors for res, _ in runs]
    assert le.is_tiled(dig) and le.is_tiled(rnd) and le.is_tiled(err)
    assert stats["systems"] == S and stats["rounds_total"] == int(rnd.astype(np.uint64).sum())
    assert stats["instructions"] == int(le.tiled(le.tile()[1]).sum())
    assert stats["err_systems"] == int(np.count_nonzero(err))
    return dig, rnd, err


# ---------------------------------------------------------------- 1. load and clear

def test_load_clears_rd_values_past_the_capped_grid(dash):
    """clear_rd_kernel over 5,120,000 chunks: its grid of 4,194,304 threads takes a second trip, over
    the systems from 32,768 on. Every RD word comes in with garbage in its value bits; what the
    device holds afterwards is the rule stated in numpy, for all 40,000 systems."""
    assert S * le.ROW > le.GRID_STRIDE_THREADS and le.GRID_STRIDE_THREADS // le.ROW == FAR[1]
    packed, lens = le.tile()
    big, big_lens = le.tiled(packed), le.tiled(lens)
    dirty = le.with_rd_garbage(big, np.random.default_rng(1))
    assert (dirty[FAR[1]:] != big[FAR[1]:]).any()
    want = np.zeros((S, N, le.MAX_INSTR), np.uint16)
    want[:, :, :le.MAXLEN] = le.clear_rd(big, big_lens)
    with big_engine(dash) as eng:
        eng.load_traces(dirty, big_lens)
        got, got_lens = eng.read_traces()
        assert np.array_equal(got_lens, big_lens)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (bad[:5], [hex(int(got[tuple(b)])) for b in bad[:5]])
        check_results_tiled(eng, eng.run())


# ---------------------------------------------------------------- 2. broadcast and explore

EXPLORE_SRC, EXPLORE_SEEDS = 32_791, 40_500


def test_broadcast_and_explore_from_a_far_source(dash):
    """broadcast_kernel's second trip, with the source inside it: every system becomes system 32,791.
    explore of that source over 40,500 seeds is two passes, the last padded with repeats, and gives
    the list of a 64-system handle over the same seeds: counts, witnesses and order."""
    assert EXPLORE_SRC >= le.GRID_STRIDE_THREADS // le.ROW and S < EXPLORE_SEEDS < 2 * S
    packed, lens = le.tile()
    j = EXPLORE_SRC % T
    assert lens[j].any()
    with big_engine(dash, schedule_seed=1) as eng:
        load_tiled(eng)
        eng.broadcast_system(EXPLORE_SRC)
        got, got_lens = eng.read_traces()
        assert (got_lens == lens[j]).all()
        assert (got[:, :, :le.MAXLEN] == le.clear_rd(packed[j:j + 1], lens[j:j + 1])).all()
        assert not got[:, :, le.MAXLEN:].any()
        outs = eng.explore(EXPLORE_SRC, 0, EXPLORE_SEEDS, cap=EXPLORE_SEEDS)
        total = eng.explore_total
    small = np.zeros((64, N, le.MAXLEN), np.uint16), np.zeros((64, N), np.uint32)
    small[0][0], small[1][0] = packed[j], lens[j]
    with dash.Engine(64, num_procs=N, cache_size=CS, max_instr=le.MAX_INSTR, schedule_seed=1) as twin:
        twin.load_traces(*small)
        want = twin.explore(0, 0, EXPLORE_SEEDS, cap=EXPLORE_SEEDS)
        assert twin.explore_total == total == len(want)
    assert outs == want
    assert sum(o["count"] for o in outs) == EXPLORE_SEEDS and 1 < len(outs)
    assert any(o["count"] > 1 for o in outs) and any(o["seed"] >= S for o in outs)  # found in the padded pass


# ---------------------------------------------------------------- 3. replicate, the default table

def test_explore_sources_over_the_large_batch(dash):
    """replicate_kernel's second trip: 13 sources copied over 40,000 systems, 3,100 seeds each in two
    passes (3,076 rows per source, then 24 fresh rows, and 12 padding systems), merged in the default
    table of 131,072 slots. Per source the list is that of explore + check_outcomes on a 64-system
    handle, every witness re-run on the oracle has the listed outcome and tests/coherence_ref.py's
    record, and per_source and the totals are sums over the list."""
    G, K = le.SRC_G, le.SRC_K
    assert S * le.ROW > le.GRID_STRIDE_THREADS and (S // G, S - G * (S // G)) == (3076, 12)
    src, src_lens = le.racy_sources()
    packed, lens = np.zeros((S, N, le.SRC_LEN), np.uint16), np.zeros((S, N), np.uint32)
    packed[:G], lens[:G] = src, src_lens
    with big_engine(dash, schedule_seed=1, keep_state=True) as eng:
        eng.load_traces(packed, lens)
        outs, per, tot = result = eng.explore_sources(G, 0, K)
        assert (tot["passes"], tot["table_slots"], tot["schedules"], tot["unplaced"]) == (2, 131_072, G * K, 0)
        assert per["schedules"].tolist() == [K] * G
        check_sums(dash, result, G)
        # the replicas past the capped grid are their sources
        got, got_lens = eng.read_traces()
        k = np.arange(S)
        assert np.array_equal(got_lens[k], src_lens[k % G]) and np.array_equal(got[k, :, :le.SRC_LEN], src[k % G])
    small = np.zeros((64, N, le.SRC_LEN), np.uint16), np.zeros((64, N), np.uint32)
    with dash.Engine(64, num_procs=N, cache_size=CS, max_instr=le.MAX_INSTR, schedule_seed=1, keep_state=True) as twin:
        for g in range(G):
            small[0][0], small[1][0] = src[g], src_lens[g]
            twin.load_traces(*small)
            old = twin.explore(0, 0, K, cap=K)
            rec = twin.check_outcomes(0, old)
            mine = outs[outs["source"] == g]
            assert [{f: int(o[f]) for f in OUT_FIELDS} for o in mine] == old, g
            assert [cr.record(o) for o in mine] == [cr.record(r) for r in rec], g
            assert len(old) > 1, g
            for o in mine:
                run = oc.run_system(src[g], src_lens[g], num_procs=N, cache_size=CS, arb_seed=int(o["seed"]),
                                    max_rounds=1024 + 256 * le.MAX_INSTR)
                assert (run.digest, run.errors, run.rounds) == (int(o["digest"]), int(o["errors"]), int(o["rounds"]))
                assert cr.record(o) == cr.check(run.node, N, CS)[0], (g, int(o["seed"]))


# ---------------------------------------------------------------- 4. coherence

def test_coherence_walk_and_grid_floor(dash):
    """coherence_kernel over 5,000 waves: the device-sized grid walks them in several trips per
    workgroup, and under DASH_TEST_ONE_GROUP the 1,250 workgroups of work exceed MAX_TRIPS, so the
    grid of one is raised to two. Both give the same records and totals: tiled, the reference's for
    the first T systems, and totals that are sums over the records."""
    blocks = -(-(S // (64 // N)) // le.COH_WAVES)
    assert blocks > le.COH_MAX_TRIPS and -(-blocks // le.COH_MAX_TRIPS) == 2
    seen = []
    for flags in (0, dash.TEST_ONE_GROUP):
        with big_engine(dash, keep_state=True, flags=flags) as eng:
            load_tiled(eng)
            stats = eng.run()
            _, _, err = check_results_tiled(eng, stats)
            tot = eng.check_coherence()
            rec = eng.read_coherence()
            assert rec.shape == (S,) and le.is_tiled(rec)
            checked = [cr.check(eng.read_state(s), N, CS) for s in range(T)]
            assert [cr.record(rec[s]) for s in range(T)] == [c[0] for c in checked] == le.tile_coherence()
            assert [cr.record(rec[s]) for s in FAR] == [checked[s % T][0] for s in FAR]
            bad = rec["bits"] != 0
            copies = np.bincount(np.arange(S) % T, minlength=T)  # systems that hold tile entry j
            assert tot == {"systems": S, "violating_systems": int(bad.sum()),
                           "violating_clean_systems": int((bad & (err == 0)).sum()),
                           "addrs": int(rec["addrs"].astype(np.uint64).sum()),
                           "bit_systems": [int(((rec["bits"] >> k) & 1).sum()) for k in range(8)],
                           "bit_addrs": [sum(int(copies[j]) * sum((b >> k) & 1 for b in checked[j][1])
                                             for j in range(T)) for k in range(8)]}
            assert 0 < tot["violating_systems"] < S and sum(b > 0 for b in tot["bit_systems"]) >= 6
            seen.append((tot, rec))
    assert seen[0][0] == seen[1][0] and np.array_equal(seen[0][1], seen[1][1])


# ---------------------------------------------------------------- 5. the event log past 4 GiB

@pytest.mark.parametrize("seed", [0, le.TILE_RNG])
def test_event_log_past_4_gib(dash, seed):
    """40,000 systems x 8 nodes x 4,096 rounds x 4 B = 5.24 GB of event log, byte 2^32 at system
    32,768: sim_kernel's writes (the lockstep event kernel, and the seeded one) and the reads of
    dash_read_events and metrics_kernel index it in 64 bits. The systems around the boundary and the
    last one hold the events of their tile entries; the first T hold the oracle's log; the metrics
    records are tiled, the reference's for the first T, and the totals are sums over them."""
    assert S * N * le.EVENT_ROUNDS * 4 > 1 << 32 and FAR[1] * N * le.EVENT_ROUNDS * 4 == 1 << 32
    runs = le.tile_runs(seed)
    with big_engine(dash, trace_events=le.EVENT_ROUNDS, schedule_seed=seed) as eng:
        load_tiled(eng)
        stats = eng.run()
        _, rounds, _ = check_results_tiled(eng, stats, seed)
        events = [events_of(eng, s) for s in range(T)]
        for s in range(T):
            assert dash.format_events(eng.read_events(s)) == runs[s][1], s
        for s in FAR:
            assert events_of(eng, s) == events[s % T] and len(events[s % T]) > 0, s
        tot = eng.compute_metrics()
        rec, cut = eng.read_metrics()
        assert rec.shape == (S, N) and le.is_tiled(rec) and not cut.any()
        for s in range(T):
            assert as_dicts(rec[s]) == mr.metrics_from_events(events[s], int(rounds[s]), N), s
        check_totals(tot, rec, cut)


# ---------------------------------------------------------------- 6. shrink: the y-stride

def test_shrink_on_more_systems_than_grid_rows(dash):
    """many_variant_kernel's gridDim.y is capped at 65,535: on 65,600 systems the last ones are written by
    the y-stride only, and check_against_twin reads the last system's traces, results and record."""
    row = sr.ROWS[1]
    N_, CS_, r, seed = row
    assert seed == 0 and le.SHRINK_Y_SYSTEMS > le.VARIANT_MAX_Y
    k, _tr, lens, bits = sr.row_source(*row)
    with shrink_engine(dash, N_, CS_, le.SHRINK_Y_SYSTEMS) as eng:
        load_shrink_batch(eng, N_, r)
        out = eng.shrink(k, bits & -bits, seed=seed)
        check_against_twin(eng, out, sr.row_twin(*row), lens, N_, CS_, seed)
        got_tr, got_ln = eng.read_traces()  # every system holds the minimal set, the y-stride's too
        assert (got_ln == got_ln[0]).all() and (got_tr == got_tr[0]).all()
        assert len(set(eng.read_results()[0].tolist())) == 1


# ---------------------------------------------------------------- 7. shrink: two x-blocks

def test_shrink_of_long_traces(dash):
    """8 nodes x 600 instructions: 152 chunks per stream, 1,216 (node, chunk) items, so many_variant_kernel
    runs two x-blocks per system, the second with the end of node 6 and all of node 7; 9,624
    candidates on 4,096 systems make three sub-passes in the first round. Steps, lengths and traces
    are the twin's (tests/golden/shrink_long.json, re-checked on the CPU)."""
    rec = le.long_fixture()
    k, tr, lens, bits = le.long_source(rec["rng"])
    W = le.write_chunks(le.LONG_M, int(lens.max()))
    assert le.LONG_N * W > le.VARIANT_ITEMS_PER_BLOCK and any(s[0] >= 6 for s in rec["twin"][2])
    packed, ln = np.zeros((le.LONG_S, le.LONG_N, le.LONG_M), np.uint16), np.zeros((le.LONG_S, le.LONG_N), np.uint32)
    packed[7], ln[7] = tr, lens
    with dash.Engine(le.LONG_S, num_procs=le.LONG_N, cache_size=le.LONG_CS, max_instr=le.LONG_M, keep_state=True,
                     schedule_seed=1) as eng:
        eng.load_traces(packed, ln)
        out = eng.shrink(7, rec["bit"], seed=0)
        check_against_twin(eng, out, rec["twin"], lens, le.LONG_N, le.LONG_CS, 0)
        Cs = [c for _, _, _, c in rec["twin"][2]] + [len(sr.candidates(out["lens"]))]
        assert Cs[0] == 9624 and out["report"]["passes"] == 2 + sum(-(-c // le.LONG_S) for c in Cs)


# ---------------------------------------------------------------- 8. ingest across slabs

def write_dirs(dash, root):
    packed, lens = le.dir_traces()
    dirs = []
    for d in range(le.DIR_DISTINCT):
        dash.write_dir(packed[d], lens[d], root / f"set{d}")
        dirs.append(root / f"set{d}")
    return dirs


def variant_dir(dash, root, name, node, text):
    """A copy of trace set 2 whose core_<node>.txt is `text` (None: missing)."""
    packed, lens = le.dir_traces()
    dash.write_dir(packed[2], lens[2], root / name)
    path = root / name / f"core_{node}.txt"
    path.unlink()
    if text is not None:
        path.write_bytes(text)
    return root / name


def test_directory_ingest_across_pinned_slabs(dash, tmp_path):
    """250 directories at max_instr 4,096 are slabs of 107, 107 and 36 systems: the third reuses the
    first's pinned buffer, and s0 offsets the files of the second and third. The device parse loads
    what the host parse loads and the run gives the same results."""
    p = le.per_slab(le.DIR_M, N, le.DIR_ENTRIES)
    assert (p, -(-le.DIR_ENTRIES // p)) == (107, 3)
    sets = write_dirs(dash, tmp_path)
    dirs = [sets[d] for d in le.dir_order()]
    with dash.Engine(le.DIR_ENTRIES, num_procs=N, cache_size=CS, max_instr=le.DIR_M) as eng:
        eng.load_dirs(dirs)
        host_tr, host_ln = eng.read_traces()
        packed, lens = le.dir_traces()
        assert np.array_equal(host_ln, lens[le.dir_order()]) and host_ln.max() == le.DIR_M  # what was written
        eng.run()
        host = [x.copy() for x in eng.read_results()]
        eng.load_dirs(dirs, device=True)
        info = eng.ingest_info()
        text = sum((d / f"core_{t}.txt").stat().st_size for d in dirs for t in range(N))
        assert info["rc"] == dash.OK and text <= info["text_bytes"] < text + 16 * N * le.DIR_ENTRIES
        got_tr, got_ln = eng.read_traces()
        assert np.array_equal(got_ln, host_ln) and np.array_equal(got_tr, host_tr)
        eng.run()
        for a, b in zip(eng.read_results(), host):
            assert np.array_equal(a, b)


BAD_PARSE = (b"RD 0x01\nWR 0x12 7\n" * 3 + b"rd 0x01\nRD 0x02\n", -3, 7)  # text, code, 1-based failing record
BAD_ADDR = (b"RD 0x01\nWR 0x12 7\nRD 0x13\nRD 0x9c\nRD 0x02\n", -4, 4)


@pytest.mark.parametrize("case", ["parse_before_missing", "missing_before_parse", "addr_before_missing"])
def test_directory_failure_across_slabs(dash, tmp_path, case):
    """The lowest failing file wins whichever slab it is in: a parse failure in slab 1 beats a missing
    file in slab 2, a missing file in slab 0 beats a parse failure in slab 1 (the later slabs are not
    read), an address failure in slab 0 beats a missing file in slab 2. file and record are exact."""
    p = le.per_slab(le.DIR_M, N, le.DIR_ENTRIES)
    sets = write_dirs(dash, tmp_path)
    dirs = [sets[d] for d in le.dir_order()]
    bad_parse = variant_dir(dash, tmp_path, "bad_parse", 3, BAD_PARSE[0])
    bad_addr = variant_dir(dash, tmp_path, "bad_addr", 1, BAD_ADDR[0])
    missing = variant_dir(dash, tmp_path, "missing", 5, None)
    if case == "parse_before_missing":
        plants, want = {150: bad_parse, 230: missing}, (dash.EPARSE, 150 * N + 3, BAD_PARSE[2])
    elif case == "missing_before_parse":
        plants, want = {50: missing, 150: bad_parse}, (dash.EIO, 50 * N + 5, 0)
    else:
        plants, want = {20: bad_addr, 230: missing}, (dash.EADDR, 20 * N + 1, BAD_ADDR[2])
    slabs = sorted(k // p for k in plants)
    assert slabs == {"parse_before_missing": [1, 2], "missing_before_parse": [0, 1],
                     "addr_before_missing": [0, 2]}[case]
    for text, code, record in (BAD_PARSE, BAD_ADDR):  # the host parser agrees about the planted files
        words, rc = dash.parse_core_text(text, N, le.DIR_M)
        assert (rc, len(words) + 1) == (code, record)
    for k, d in plants.items():
        dirs[k] = d
    with dash.Engine(le.DIR_ENTRIES, num_procs=N, cache_size=CS, max_instr=le.DIR_M) as eng:
        with pytest.raises(dash.DashError) as ei:
            eng.load_dirs(dirs, device=True)
        info = eng.ingest_info()
        assert (ei.value.code, info["rc"], info["file"], info["record"]) == (want[0], *want)
        assert str(dirs[want[1] // N]) in str(ei.value) and f"node {want[1] % N}" in str(ei.value)
        with pytest.raises(dash.DashError) as ei:
            eng.run()
        assert ei.value.code == dash.ESTATE


# ---------------------------------------------------------------- 9. mark

def test_overflow_hint_of_more_systems_than_the_mark_grid(dash):
    """300,000 copies of a system deeper than 32 on a handle that starts at the 32-deep tier: every
    system overflows, so mark_kernel marks 300,000 list entries with a grid capped at 262,144
    threads, and the second run takes the hinted route (all systems at 256 on the side stream, all
    skipped by the first tier). Both runs give the oracle's results for every system, and
    tier_systems follows test_overflow_hint_against_the_oracle's rule in both."""
    import bench_next
    n = le.MARK_SYSTEMS
    assert n > le.MARK_THREADS
    L = 200
    packed, lens = contended(8, 1, L)
    ref = contended_oracle(8, 1, L, 0)
    depth = depth_of(ref)
    s = int(np.argmax(depth))
    assert depth[s] > 32
    res = ref[s]
    slab, off, ln = dash.pack_text([bench_next.trace_text(packed[s, t, :lens[s, t]]) for t in range(8)])
    expect = tier_counts(np.full(n, depth[s]), first=1)
    assert expect == [0, n, n]
    with dash.Engine(n, num_procs=8, cache_size=1, max_instr=L, flags=dash.TIER_FROM_32) as eng:
        eng.load_text_slab(slab, np.tile(off, n), np.tile(ln, n))
        for run in range(2):
            stats = eng.run()
            dig, rnd, err = eng.read_results()
            assert (dig == res.digest).all() and (rnd == res.rounds).all() and (err == res.errors).all(), run
            assert stats["tier_systems"] == expect, run
            assert stats["hist"] == [n * int(x) for x in res.hist] and stats["instructions"] == n * res.instructions
            assert stats["systems"] == n and stats["rounds_total"] == n * res.rounds
            assert stats["max_depth"] == res.max_depth and stats["dropped"] == n * res.dropped


# ---------------------------------------------------------------- 10. the digest file's windows

def test_digest_file_second_window(dash, tmp_path):
    """dash_write_digests formats windows of 2 x 16 chunks of 65,536 lines: 2,167,152 systems are one
    full window and a second one of a full and a partial chunk. Line for line the formatted
    dash_read_results."""
    if len(os.sched_getaffinity(0)) < le.DIGEST_THREADS:
        pytest.skip(f"host_threads gives fewer than {le.DIGEST_THREADS} threads on this machine: "
                    "the window would not be 2 x 16 chunks")
    n = le.DIGEST_SYSTEMS
    assert n > 2 * le.DIGEST_THREADS * le.DIGEST_CHUNK
    with dash.Engine(n, num_procs=1, cache_size=4, max_instr=8) as eng:
        eng.generate(0x5EED, 8, kind=dash.GEN_UNIFORM)
        eng.run()
        dig, rnd, err = eng.read_results()
        eng.write_digests(tmp_path / "d.txt")
    assert len(set(dig[-1000:].tolist())) > 1
    rows = enumerate(zip(dig.tolist(), rnd.tolist(), err.tolist()))
    exp = "".join(f"{k} {d:016x} {r} {e:x}\n" for k, (d, r, e) in rows)
    got = (tmp_path / "d.txt").read_text()
    assert len(got) == len(exp) and got == exp
