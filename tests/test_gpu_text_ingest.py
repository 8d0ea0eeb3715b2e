"""Trace text parsed on the GPU (dash_load_text, dash_load_dirs_device,
csrc/dash_ingest.hip) against the host parser: dash_parse_core_text, which
test_text_parse.py pins to dash_parse_core_file. Every input here is one the
host parser handles; what the device leaves in the simulator's layout is read
back with dash_read_traces and compared word for word.

Cap features on tile edges: with max_instr 2,048 the record that reaches the cap
cannot start before byte 4 * 2,047 = 2T - 4 (a record is at least 4 bytes, "RD1\\n"),
so at that cap the cap cases cover offsets [2T - 4, 2T + 20]; the remaining offsets
of both windows and the wave boundaries run the same cases at smaller caps (300, 600,
76, 150, 225), where the arithmetic allows them. Nothing is left out.
"""
import subprocess

import numpy as np
import pytest

import text_corpus as tc
from oracle_ctypes import GOLDEN

pytestmark = pytest.mark.gpu
TESTS = ["sample", "test_1", "test_2", "test_3", "test_4"]
EXPECT = {"sample": "", "test_1": "", "test_2": "", "test_3": "run_1", "test_4": "run_1"}


def expected(dash, blobs, num_procs, max_instr):
    """(packed, lens, codes) of dash_parse_core_text over blobs[system][node]."""
    nsys = len(blobs)
    packed = np.zeros((nsys, num_procs, max(max_instr, 1)), dtype=np.uint16)
    lens = np.zeros((nsys, num_procs), dtype=np.uint32)
    codes = np.zeros((nsys, num_procs), dtype=np.int32)
    for s, row in enumerate(blobs):
        for t, data in enumerate(row):
            words, rc = dash.parse_core_text(data, num_procs, max_instr)
            packed[s, t, :len(words)] = words
            lens[s, t] = len(words)
            codes[s, t] = rc
    return packed, lens, codes


def check_loaded(eng, want_packed, want_lens):
    packed, lens = eng.read_traces()
    assert np.array_equal(lens, want_lens), np.argwhere(lens != want_lens)[:5]
    bad = np.argwhere(packed != want_packed)
    assert len(bad) == 0, (bad[:5], [hex(int(packed[tuple(b)])) for b in bad[:5]])


# ---------------------------------------------------------------- 1. corpus parity

@pytest.mark.parametrize("num_procs", [4, 8, 3])
def test_corpus_parity(dash, num_procs):
    nsys, M = 375, 32  # 375 is no multiple of 64 / seg; at N = 3 a system's lanes are padded (seg 4)
    good = tc.accepted(dash, num_procs, M)
    assert len(good) >= 500
    files = tc.corpus()
    blobs = [[files[good[(s * num_procs + t) % len(good)][0]] for t in range(num_procs)] for s in range(nsys)]
    want_packed, want_lens, codes = expected(dash, blobs, num_procs, M)
    assert not codes.any() and want_lens.max() == M and want_lens.min() == 0
    with dash.Engine(nsys, num_procs=num_procs, max_instr=M) as eng:
        eng.load_text(blobs)
        info = eng.ingest_info()
        assert info["rc"] == dash.OK and info["text_bytes"] > 0
        check_loaded(eng, want_packed, want_lens)


# ---------------------------------------------------------------- 2. failure selection

def _valid(i):
    return b"WR 0x%02x %d\n" % ((i * 7) % 48, i % 256) if i % 2 else b"RD 0x%02x\n" % ((i * 5) % 48)


def _planted(record, bad):
    """A file whose 1-based record `record` is `bad`, among valid ones."""
    return b"".join(_valid(i) for i in range(record - 1)) + bad + b"".join(_valid(i) for i in range(5))


@pytest.mark.parametrize("plants,winner", [
    ([(5, 2, 7, b"rd 0x01\n", -3)], 0),
    ([(63, 3, 1, b"RD 0x40\n", -4)], 0),
    ([(0, 0, 32, b"\n", -3)], 0),
    ([(40, 1, 3, b"WR 0x7f 1\n", -4), (12, 0, 32, b"WR 0x12\n", -3)], 1),   # the lower file wins
    ([(9, 3, 2, b"RD zz\n", -3), (9, 2, 30, b"RD 0xff\n", -4), (50, 0, 1, b"", -3)], 1),
])
def test_failure_selection(dash, plants, winner):
    nsys, N, M = 64, 4, 32
    blobs = [[b"".join(_valid(s + t + i) for i in range((s * 5 + t) % 33)) for t in range(N)] for s in range(nsys)]
    for s, t, record, bad, _ in plants:
        blobs[s][t] = _planted(record, bad) if bad else b"\n"
    s, t, record, _, code = plants[winner]
    _, _, codes = expected(dash, blobs, N, M)
    assert codes[s, t] == code and sorted(zip(*np.nonzero(codes)))[0] == (s, t)  # the host parser agrees
    with dash.Engine(nsys, num_procs=N, max_instr=M) as eng:
        with pytest.raises(dash.DashError) as ei:
            eng.load_text(blobs)
        assert ei.value.code == code
        assert f"system {s}" in str(ei.value) and f"node {t}" in str(ei.value) and f"record {record}" in str(ei.value)
        info = eng.ingest_info()
        assert (info["rc"], info["file"], info["system"], info["node"], info["record"]) == (code, s * N + t, s, t, record)
        with pytest.raises(dash.DashError) as ei:  # written in place: not loaded after a failure
            eng.run()
        assert ei.value.code == dash.ESTATE
        with pytest.raises(dash.DashError) as ei:
            eng.read_traces()
        assert ei.value.code == dash.ESTATE
        # and a good batch loads on the same handle afterwards
        for ps, pt, _, _, _ in plants:
            blobs[ps][pt] = _valid(1)
        eng.load_text(blobs)
        assert eng.ingest_info()["rc"] == dash.OK
        check_loaded(eng, *expected(dash, blobs, N, M)[:2])
        eng.run()


# ---------------------------------------------------------------- 3. tile and wave edges

def _line(i, n):
    """A valid record of exactly n bytes (4 <= n <= 19), newline included; its word depends on i."""
    if n >= 12 and i % 2:
        body = b"WR 0x%02x %d" % ((i * 7) % 48, i % 256)
        return body + b" " * (n - 1 - len(body)) + b"\n"
    hexd = b"%x" % (i % 16) if n == 4 else b"%02x" % ((i * 5) % 48)
    return b"RD" + b" " * (n - 3 - len(hexd)) + hexd + b"\n"


def fill(nbytes, first=0):
    """Valid lines of 8..19 bytes, exactly nbytes in all (0 or >= 8)."""
    out, i = [], first
    while nbytes:
        assert nbytes >= 8
        if nbytes <= 19:
            n = nbytes
        else:
            n = 8 + (i * 5) % 12
            if nbytes - n < 8:      # leave a last line of 8: nbytes < 27 here, so 12 <= n <= 18
                n = nbytes - 8
        out.append(_line(i, n))
        nbytes -= n
        i += 1
    return b"".join(out)


def fill_exact(nbytes, nrec):
    """Exactly nrec valid records in exactly nbytes (4 * nrec <= nbytes <= 19 * nrec)."""
    assert 4 * nrec <= nbytes <= 19 * nrec, (nbytes, nrec)
    base, extra = divmod(nbytes, nrec)
    return b"".join(_line(i, base + (1 if i < extra else 0)) for i in range(nrec))


TAIL = fill(45, first=3)
CHUNK19 = b"WR 0x1e 201".ljust(19)  # a full 19-byte chunk without newline: one record


def ok_features(X):
    """Files the parser accepts, each with one feature at byte offset X."""
    return {
        "newline": fill(X + 1) + TAIL,
        "chunk": fill(X - 19) + CHUNK19 + b"RD 0x05\n" + TAIL,           # the second chunk starts at X
        "chunk3": fill(X - 38) + CHUNK19 + CHUNK19 + b"RD\t0x06\n" + TAIL,
        "nul": fill(X - 7) + b"RD 0x12\0zz\n" + TAIL,                     # the NUL sits at X
    }


def cap_features(X, M):
    """The record that reaches the cap starts at X: alone, and with bad text right after it."""
    head = fill_exact(X, M - 1)
    return {"cap": head + b"WR 0x2a 77\n" + TAIL,
            "cap_then_bad": head + b"WR 0x2a 77\nbad\n\nRD 0xff\n" + TAIL}


def bad_features(X, M, plain):
    """Failures at X: name -> (file, code). plain: those that need no cap (X lies before it)."""
    out = {}
    if plain:
        out = {"nul_before_value": (fill(X - 7) + b"WR 0x12\0 5\n" + TAIL, -3),
               "empty_line": (fill(X) + b"\n" + TAIL, -3)}
    if 4 * (M - 1) <= X <= 19 * (M - 1):  # the last record the cap admits is bad: it must win
        out["bad_at_cap"] = (fill_exact(X, M - 1) + b"bad\n" + TAIL, -3)
        out["addr_at_cap"] = (fill_exact(X, M - 1) + b"RD 0x9c\n" + TAIL, -4)
    return out


def _windows(dash):
    T = dash.TEXT_TILE
    w1 = list(range(T - 20, T + 21))
    w2 = list(range(2 * T - 20, 2 * T + 21))
    waves = [k * T // 4 + d for k in (1, 2, 3) for d in (-1, 0, 1)]
    return T, w1, w2, waves


def edge_groups(dash):
    """max_instr -> (offsets for the plain features, offsets for the cap features)."""
    T, w1, w2, waves = _windows(dash)
    return {2048: (w1 + w2 + waves, [x for x in w2 if x >= 4 * 2047]),
            300: ([], w1), 600: ([], w2),
            76: ([], waves[0:3]), 150: ([], waves[3:6]), 225: ([], waves[6:9])}


@pytest.mark.parametrize("max_instr", [2048, 300, 600, 76, 150, 225])
def test_tile_and_wave_edges(dash, max_instr):
    N, M = 4, max_instr
    T = dash.TEXT_TILE
    assert T == 4096
    plain, capped = edge_groups(dash)[M]
    files = []
    for X in plain:
        files += list(ok_features(X).values())
    for X in capped:
        files += list(cap_features(X, M).values())
    if M == 2048:
        files += [b"", b"RD1\n" * 2048, b"RD1\n" * 3000, fill(3 * T + 5)]
    while len(files) % N:
        files.append(b"")
    blobs = [files[i:i + N] for i in range(0, len(files), N)]
    want_packed, want_lens, codes = expected(dash, blobs, N, M)
    assert not codes.any()
    if capped:
        assert (want_lens == M).sum() >= 2 * len(capped)
    with dash.Engine(len(blobs), num_procs=N, max_instr=M) as eng:
        eng.load_text(blobs)
        check_loaded(eng, want_packed, want_lens)
        # the same files at unaligned offsets inside one slab (gaps of 1, 3, 7, ... bytes of junk)
        slab, off = bytearray(b"RD"), []
        for k, f in enumerate(files):
            slab += b"\nWR 0x99 bad"[:1 + (k * 2) % 11]
            off.append(len(slab))
            slab += f
        eng.load_text_slab(bytes(slab), np.array(off, dtype=np.uint64), np.array([len(f) for f in files], dtype=np.uint32))
        assert sum(o % 16 != 0 for o in off) > len(off) // 2
        check_loaded(eng, want_packed, want_lens)
    # failures, one call each on a one-system handle: the failing file sits at node 2
    cases = []
    for X in sorted(set(plain) | set(capped)):
        cases += [(name, f, code) for name, (f, code) in bad_features(X, M, X in plain).items()]
    assert sum(name == "bad_at_cap" for name, _, _ in cases) == len(capped)
    if M == 2048:
        cases += [("one_byte", b"R", -3), ("one_newline", b"\n", -3), ("only_newlines", b"\n" * 5000, -3),
                  ("nul_only", b"\0", -3)]
    with dash.Engine(1, num_procs=N, max_instr=M) as eng:
        for name, f, code in cases:
            words, rc = dash.parse_core_text(f, N, M)
            assert rc == code, name
            with pytest.raises(dash.DashError) as ei:
                eng.load_text([[fill(40), fill(T + 3), f, b""]])
            info = eng.ingest_info()
            assert (ei.value.code, info["file"], info["record"]) == (code, 2, len(words) + 1), (name, len(f))


# ---------------------------------------------------------------- 4. directories

def test_directories(dash, tmp_path):
    dirs = [GOLDEN / TESTS[k % 5] for k in range(40)]
    with dash.Engine(40, num_procs=4, cache_size=4, max_instr=32, keep_state=True) as eng:
        eng.load_dirs(dirs)
        host_traces = eng.read_traces()
        eng.run()
        host = eng.read_results()
        eng.load_dirs(dirs, device=True)
        info = eng.ingest_info()
        assert info["rc"] == dash.OK
        text = sum((d / f"core_{t}.txt").stat().st_size for d in dirs for t in range(4))
        assert text <= info["text_bytes"] < text + 16 * 160  # bytes copied: files start on 16-byte boundaries
        check_loaded(eng, *host_traces)
        eng.run()
        for a, b in zip(eng.read_results(), host):
            assert np.array_equal(a, b)
        for k in (0, 1, 2, 3, 4, 37, 39):
            eng.dump_system(k, tmp_path / str(k))
            exp = GOLDEN / TESTS[k % 5] / EXPECT[TESTS[k % 5]]
            for n in range(4):
                assert (tmp_path / str(k) / f"core_{n}_output.txt").read_bytes() == (exp / f"core_{n}_output.txt").read_bytes()


def test_directories_missing_file(dash, tmp_path, capfd):
    dirs = []
    for k in range(12):
        d = tmp_path / f"s{k}"
        d.mkdir()
        for t in range(4):
            (d / f"core_{t}.txt").write_bytes((GOLDEN / "sample" / f"core_{t}.txt").read_bytes())
        dirs.append(d)
    (dirs[7] / "core_2.txt").unlink()
    (dirs[9] / "core_0.txt").write_bytes(b"oops\n")          # a later parse failure does not win
    with dash.Engine(12, num_procs=4, max_instr=32) as eng:
        with pytest.raises(dash.DashError) as ei:
            eng.load_dirs(dirs, device=True)
        assert ei.value.code == dash.EIO and str(dirs[7]) in str(ei.value) and "node 2" in str(ei.value)
        info = eng.ingest_info()
        assert (info["rc"], info["file"], info["record"]) == (dash.EIO, 7 * 4 + 2, 0)
        with pytest.raises(dash.DashError) as ei:
            eng.run()
        assert ei.value.code == dash.ESTATE
        (dirs[3] / "core_1.txt").write_bytes(b"RD 0x01\nWR 0x55 1\n")  # an earlier parse failure does
        with pytest.raises(dash.DashError) as ei:
            eng.load_dirs(dirs, device=True)
        assert ei.value.code == dash.EADDR and str(dirs[3]) in str(ei.value)
        info = eng.ingest_info()
        assert (info["rc"], info["file"], info["record"]) == (dash.EADDR, 3 * 4 + 1, 2)
    assert "count not open file" in capfd.readouterr().err


def test_cli_device_ingest(dash, tmp_path):
    exe = dash.PKG / "cache_simulator"
    lst = tmp_path / "dirs.txt"
    lst.write_text("\n".join(str(GOLDEN / TESTS[k % 5]) for k in range(15)) + "\n")
    outs = []
    for name, extra in (("host", []), ("device", ["--device-ingest"])):
        p = subprocess.run([str(exe), "--batch", str(lst), "-o", str(tmp_path / name), "--digests",
                            str(tmp_path / f"{name}.txt")] + extra, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        outs.append((tmp_path / f"{name}.txt").read_bytes())
    assert outs[0] == outs[1] and outs[0].count(b"\n") == 15
    for n in range(4):
        assert (tmp_path / "device" / "14" / f"core_{n}_output.txt").read_bytes() == \
            (tmp_path / "host" / "14" / f"core_{n}_output.txt").read_bytes()


# ---------------------------------------------------------------- 5. existing paths afterwards

def test_existing_paths_after_device_ingest(dash):
    nsys, N, M = 96, 8, 64
    rng = np.random.default_rng(11)
    packed = (rng.integers(0, 1 << 15, (nsys, N, M)) | (rng.integers(0, 2, (nsys, N, M)) << 15)).astype(np.uint16)
    lens = rng.integers(0, M + 1, (nsys, N)).astype(np.uint32)
    import bench_next
    blobs = [[bench_next.trace_text(packed[s, t, :lens[s, t]]) for t in range(N)] for s in range(nsys)]
    with dash.Engine(nsys, num_procs=N, max_instr=M) as ref:
        ref.load_traces(packed, lens)
        ref.run()
        want = ref.read_results()
        ref.generate(0x5EED, M)
        ref.run()
        want_gen = ref.read_results()
    with dash.Engine(nsys, num_procs=N, max_instr=M) as eng:
        eng.load_traces(packed, lens)
        eng.run()          # a run first, so that an overflow hint may exist when the text arrives
        eng.load_text(blobs)
        got_packed, got_lens = eng.read_traces()
        assert np.array_equal(got_lens, lens)
        rd = (packed & 0x8000) == 0
        canon = np.where(rd, packed & 0xFF00, packed)  # an RD carries value 0 (dash.h)
        canon[np.arange(M)[None, None, :] >= lens[:, :, None]] = 0
        assert np.array_equal(got_packed, canon)
        with pytest.raises(dash.DashError) as ei:
            eng.read_results()                         # ran is cleared by the load
        assert ei.value.code == dash.ESTATE
        eng.run()
        for a, b in zip(eng.read_results(), want):
            assert np.array_equal(a, b)
        eng.load_traces(packed, lens)                  # and the older loaders still work after it
        eng.run()
        for a, b in zip(eng.read_results(), want):
            assert np.array_equal(a, b)
        eng.generate(0x5EED, M)
        eng.run()
        for a, b in zip(eng.read_results(), want_gen):
            assert np.array_equal(a, b)
