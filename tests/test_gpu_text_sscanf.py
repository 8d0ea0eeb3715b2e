"""The device trace-text parser (parse_record, csrc/dash_ingest.hip) against the C library's
sscanf: tests/sscanf_ref.py, the twin that test_text_sscanf.py holds the host parsers to.
test_gpu_text_ingest.py compares the device with dash_parse_core_text on text both were written
for; here the inputs are the classes where a hand-written scanner and the library once parted
(DESIGN.md §5.3), and every expected word, code and record number is the twin's.

The tile edge is the smallest shape at which parse_record's `lim` and the halo can differ from
the host: a record that starts before the tile's end and whose deciding byte -- the sign, the
'\\r' between the tokens, the x of a digitless 0x, the 17th hex digit -- lies at offset X, for
every X within 20 bytes of the first tile boundary.
"""
import numpy as np
import pytest

import sscanf_ref as twin
import text_corpus as tc
from test_gpu_text_ingest import TAIL, check_loaded, expected, fill, fill_exact

pytestmark = pytest.mark.gpu


def expected_twin(blobs, num_procs, max_instr):
    """(packed, lens, codes) of the twin over blobs[system][node]."""
    nsys = len(blobs)
    packed = np.zeros((nsys, num_procs, max(max_instr, 1)), dtype=np.uint16)
    lens = np.zeros((nsys, num_procs), dtype=np.uint32)
    codes = np.zeros((nsys, num_procs), dtype=np.int32)
    for s, row in enumerate(blobs):
        for t, data in enumerate(row):
            words, rc = twin.parse_core_text(data, num_procs, max_instr)
            packed[s, t, :len(words)] = words
            lens[s, t] = len(words)
            codes[s, t] = rc
    return packed, lens, codes


def both(dash, blobs, num_procs, max_instr):
    """The twin's (packed, lens) for accepted files, which dash_parse_core_text must share."""
    want_packed, want_lens, codes = expected_twin(blobs, num_procs, max_instr)
    host_packed, host_lens, host_codes = expected(dash, blobs, num_procs, max_instr)
    assert not codes.any() and not host_codes.any()
    assert np.array_equal(host_lens, want_lens) and np.array_equal(host_packed, want_packed)
    return want_packed, want_lens


@pytest.mark.parametrize("num_procs", [4, 8, 3])
def test_second_corpus_parity(dash, num_procs):
    nsys, M = 375, 32
    good = tc.scanf_accepted(twin, num_procs, M)
    assert len(good) >= 500
    files = tc.scanf_corpus()
    blobs = [[files[good[(s * num_procs + t) % len(good)][0]] for t in range(num_procs)] for s in range(nsys)]
    want_packed, want_lens = both(dash, blobs, num_procs, M)
    assert want_lens.max() == M and want_lens.min() == 0
    with dash.Engine(nsys, num_procs=num_procs, max_instr=M) as eng:
        eng.load_text(blobs)
        assert eng.ingest_info()["rc"] == dash.OK
        check_loaded(eng, want_packed, want_lens)


# (bytes of the record before its deciding byte, the record): accepted by the library
OK_AT = {
    "sign": (3, b"WR -0xee 7\n"),
    "sign_rd": (2, b"RD+0X1e\n"),
    "blank": (7, b"WR 0x12\r5\n"),
    "digitless_0x": (4, b"WR 0x 5\n"),
    "digit_17": (18, b"RD00000000000000012" b"RD 0x05\n"),  # 19 bytes without newline, then the next record
}
# rejected by the library, or parsed to an address no node of 4 homes
BAD_AT = {
    "lone_sign": (3, b"RD -\n"),
    "sign_then_g": (3, b"RD +g\n"),
    "blank_then_end": (5, b"WR 1 \r\n"),
    "wr_lone_sign": (3, b"WR -\n"),
    "digitless_0x_then_g": (4, b"WR 0xg 5\n"),
    "saturated": (18, b"RD10000000000000012" b"RD 0x05\n"),
    "negative": (3, b"RD -0x10\n"),
}


# A record that ends at its '\n' before a number is complete, followed by a line a scan that
# stepped over the '\n' would take for the number: on the device the next line's bytes lie below
# parse_record's `lim` (19 bytes on), in the host's line buffer they do not. (offset of the
# '\n', the text): the library rejects the first record of each.
TRUNCATED_AT = {
    "rd_then_digits": (2, b"RD\n12\n"),
    "rd_blank_then_0x": (3, b"RD \n0x21\n"),
    "rd_crlf_then_0x": (4, b"RD \r\n0x21\n"),
    "rd_sign_then_digit": (4, b"RD -\n1\n"),
    "wr_then_both": (2, b"WR\n1 5\n"),
    "wr_then_value": (7, b"WR 0x12\n5\n"),
    "wr_crlf_then_value": (6, b"WR 1 \r\n7\n"),
    "wr_sign_then_value": (6, b"WR 1 -\n7\n"),
    "wr_then_blank_value": (5, b"WR 2e\n\t+9\n"),
}


def _window(dash):
    T = dash.TEXT_TILE
    return list(range(T - 20, T + 21))


def test_new_classes_at_the_tile_edge(dash):
    N, M = 4, 2048
    files = []
    for X in _window(dash):
        for k, rec in OK_AT.values():
            files.append(fill(X - k) + rec + TAIL)
            assert files[-1][X] == rec[k] and rec[k] in b"-+\rx2"
    while len(files) % N:
        files.append(b"")
    blobs = [files[i:i + N] for i in range(0, len(files), N)]
    want_packed, want_lens = both(dash, blobs, N, M)
    with dash.Engine(len(blobs), num_procs=N, max_instr=M) as eng:
        eng.load_text(blobs)
        check_loaded(eng, want_packed, want_lens)
        # the same files at unaligned offsets inside one slab (gaps of 1, 3, 5, ... bytes of junk)
        slab, off = bytearray(b"RD"), []
        for k, f in enumerate(files):
            slab += b"\nWR 0x99 bad"[:1 + (k * 2) % 11]
            off.append(len(slab))
            slab += f
        assert sum(o % 16 != 0 for o in off) > len(off) // 2
        eng.load_text_slab(bytes(slab), np.array(off, dtype=np.uint64), np.array([len(f) for f in files], dtype=np.uint32))
        check_loaded(eng, want_packed, want_lens)


def test_failure_selection_of_the_new_classes(dash):
    """One call each on a one-system handle, the failing file at node 2 among valid ones: code,
    file and record are the twin's."""
    N, M = 4, 2048
    T = dash.TEXT_TILE
    cases = [(name, X, fill(X - k) + rec + TAIL) for X in _window(dash) for name, (k, rec) in BAD_AT.items()]
    cases += [(name, 0, fill(40) + rec + TAIL) for name, (_, rec) in BAD_AT.items()]
    codes = set()
    with dash.Engine(1, num_procs=N, max_instr=M) as eng:
        for name, X, f in cases:
            words, rc = twin.parse_core_text(f, N, M)
            assert rc in (dash.EPARSE, dash.EADDR), name
            codes.add(rc)
            assert dash.parse_core_text(f, N, M)[1] == rc and len(dash.parse_core_text(f, N, M)[0]) == len(words)
            with pytest.raises(dash.DashError) as ei:
                eng.load_text([[fill(40), fill(T + 3), f, b""]])
            info = eng.ingest_info()
            assert (ei.value.code, info["file"], info["record"]) == (rc, 2, len(words) + 1), (name, X)
    assert codes == {dash.EPARSE, dash.EADDR}


@pytest.mark.parametrize("max_instr", [2048, 300, 1])
def test_no_scan_leaves_its_record(dash, max_instr):
    """TRUNCATED_AT with the '\\n' at every offset around the tile edge: mid-file (cap 2,048), as
    the record that reaches the cap (cap 300: 299 records before it, so that a scan which took
    the next line for the number would load the file whole), and as a file's only record (cap
    1). Code, file and record are the twin's."""
    N, M = 4, max_instr
    T = dash.TEXT_TILE
    if M == 2048:
        cases = [(name, X, fill(X - k) + text + TAIL) for X in _window(dash) for name, (k, text) in TRUNCATED_AT.items()]
    elif M == 300:  # 4 * 299 <= X - k <= 19 * 299 for every X of the window
        cases = [(name, X, fill_exact(X - k, M - 1) + text + TAIL) for X in _window(dash)
                 for name, (k, text) in TRUNCATED_AT.items()]
    else:
        cases = [(name, k, text) for name, (k, text) in TRUNCATED_AT.items()]
    with dash.Engine(1, num_procs=N, max_instr=M) as eng:
        for name, X, f in cases:
            assert f[X:X + 1] == b"\n"
            words, rc = twin.parse_core_text(f, N, M)
            assert rc == dash.EPARSE and (M == 2048 or len(words) == M - 1), name
            assert dash.parse_core_text(f, N, M)[1] == rc and len(dash.parse_core_text(f, N, M)[0]) == len(words)
            with pytest.raises(dash.DashError) as ei:
                eng.load_text([[fill(40), fill(T + 3), f, b""]])
            info = eng.ingest_info()
            assert (ei.value.code, info["file"], info["record"]) == (rc, 2, len(words) + 1), (name, X)


def test_enumeration_on_the_device(dash):
    """The exhaustive part of the enumeration, one record per file, N = 8: the files the twin
    accepts in one batch, word for word; of those it rejects, the ones in which a '\\n' is
    followed by more text (where the device's `lim` reaches past the record's end and the host's
    line buffer does not), one call each: all with up to 3 bytes after the opcode and every fifth
    with 4, so that the test stays within seconds. Code and record are the twin's."""
    N, M = 8, 32
    recs, exhaustive = tc.enumeration()
    recs = recs[:exhaustive]
    verdict = [twin.parse_core_text(r, N, M) for r in recs]
    good = [r for r, (_, rc) in zip(recs, verdict) if rc == twin.OK]
    bad = [(r, len(w), rc) for r, (w, rc) in zip(recs, verdict) if rc != twin.OK and b"\n" in r[:-1]]
    bad = [b for b in bad if len(b[0]) <= 5] + [b for b in bad if len(b[0]) == 6][::5]  # all up to 3 bytes, a fifth of the 4s
    assert len(good) >= 5000 and len(bad) >= 3000 and {rc for _, _, rc in bad} == {dash.EPARSE, dash.EADDR}
    while len(good) % N:
        good.append(b"")
    blobs = [good[i:i + N] for i in range(0, len(good), N)]
    want_packed, want_lens = both(dash, blobs, N, M)
    with dash.Engine(len(blobs), num_procs=N, max_instr=M) as eng:
        eng.load_text(blobs)
        check_loaded(eng, want_packed, want_lens)
    with dash.Engine(1, num_procs=N, max_instr=M) as eng:
        for r, n, rc in bad:
            with pytest.raises(dash.DashError) as ei:
                eng.load_text([[b"", b"RD 1\n", r, b"", b"", b"", b"", b""]])
            info = eng.ingest_info()
            assert (ei.value.code, info["file"], info["record"]) == (rc, 2, n + 1), r
