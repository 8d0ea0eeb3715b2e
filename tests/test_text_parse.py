"""dash_parse_core_text (the in-memory restatement of dash_parse_core_file, and
the oracle of the device parser) and dash_read_dirs_text, CPU only.

The corpus (text_corpus.py) is judged by dash_parse_core_file alone first, so
a generator that stops producing a class of input fails here instead of
letting the comparison go quiet."""
import numpy as np
import pytest

import sscanf_ref
import text_corpus as tc
from oracle_ctypes import GOLDEN


@pytest.fixture(scope="module")
def on_disk(dash, tmp_path_factory):
    """The corpus as files (written once), and the file parser's verdicts at N = 4, cap 32."""
    root = tmp_path_factory.mktemp("corpus")
    paths = []
    for i, data in enumerate(tc.corpus()):
        p = root / f"f{i}.txt"
        p.write_bytes(data)
        paths.append(p)
    return paths


def test_corpus_covers_every_class(dash, on_disk):
    files = tc.corpus()
    assert len(files) == 3000 and all(d.count(b"\n") <= 80 for d in files)
    ok = eparse = eaddr = capped = split = 0
    for data, path in zip(files, on_disk):
        words, rc = tc.parse_file(dash, path, 4, 32)
        full, rc_full = tc.parse_file(dash, path, 4, 4096)
        ok += rc == dash.OK
        eparse += rc == dash.EPARSE
        eaddr += rc == dash.EADDR
        # cut by the cap: accepted at 32 records although bad text follows them
        capped += rc == dash.OK and len(words) == 32 and rc_full != dash.OK
        # a long line whose chunks are accepted: more records than line ends before the stop
        rec = 0  # records before the current line (a line of b bytes is ceil(b / 19) records)
        for ln in data.splitlines(keepends=True) if b"\r" not in data else []:
            chunks = -(-len(ln) // 19)
            if chunks >= 2 and rec + 2 <= len(full):
                split += 1
                break
            rec += chunks
            if rec >= len(full):
                break
    assert ok >= 100 and eparse >= 100 and eaddr >= 100 and capped >= 100, (ok, eparse, eaddr, capped)
    assert split >= 20, split


@pytest.mark.parametrize("num_procs", [3, 4, 8])
@pytest.mark.parametrize("max_instr", [0, 1, 32])
def test_text_equals_file_parser(dash, on_disk, num_procs, max_instr):
    for data, path in zip(tc.corpus(), on_disk):
        want, want_rc = tc.parse_file(dash, path, num_procs, max_instr)
        got, got_rc = dash.parse_core_text(data, num_procs, max_instr)
        assert got_rc == want_rc and got.tolist() == want.tolist(), (path.name, data)


def test_rules_spelled_out(dash):
    P = lambda s, n=4, m=32: (lambda w, rc: (w.tolist(), rc))(*dash.parse_core_text(s, n, m))
    assert P(b"RD 0x\n") == ([0x0000], dash.OK)                   # "0x" without a digit: the 0 is the number
    # where a hand-written scanner and the library's sscanf once parted: a sign on
    # the hex number, any isspace byte as a blank, a 0x consumed without a digit, saturation at 17
    # significant hex digits. What each reads is the library's own answer (sscanf_ref.py).
    S = lambda s, n=4, m=32: (lambda w, rc: (w.tolist(), rc))(*sscanf_ref.parse_core_text(s, n, m))
    for rec in (b"RD -1\n", b"RD +1f\n", b"RD -0x10\n", b"RD -0xee\n", b"WR -0xff +3\n",
                b"WR 0x12\r5\n", b"WR\f0x12 5\n", b"WR 0x12\v7\n", b"RD\r0x21\n",
                b"WR 0x 5\n", b"WR 0X-5\n", b"WR 0xg 5\n", b"RD 0x\0junk\n",
                b"RD12345678901234567", b"RDffffffffffffffff1", b"RD00000000000000012", b"RD-ffffffffffffffef"):
        for n in (4, 8):
            assert P(rec, n) == S(rec, n), (rec, n)
    assert S(b"RD -0xee\n")[1] == S(b"WR 0x 5\n")[1] == S(b"WR 0x12\r5\n")[1] == dash.OK
    assert S(b"RDffffffffffffffff1")[1] == dash.EADDR and S(b"WR 0xg 5\n")[1] == dash.EPARSE
    assert P(b"WR 0x15 300\nRD 17\n") == ([0x8000 | 0x1500 | 44, 0x1700], dash.OK)
    assert P(b"WR 0x15 -1") == ([0x8000 | 0x1500 | 255], dash.OK)  # no final newline
    assert P(b"\n") == ([], dash.EPARSE)
    assert P(b"") == ([], dash.OK)
    assert P(b"RD 0x12\0zz\nRD 0x13\n") == ([0x1200, 0x1300], dash.OK)   # NUL ends content, not extent
    assert P(b"WR 0x12\0 5\n") == ([], dash.EPARSE)
    assert P(b"WR 0x45 x\n") == ([], dash.EPARSE)                 # a WR without value: parse, not address
    assert P(b"RD 0x45\n") == ([], dash.EADDR)
    assert P(b"RD 0x45\n", 8) == ([0x4500], dash.OK)
    assert P(b"RD 0x01\nbad\n", 4, 1) == ([0x0100], dash.OK)      # nothing past the cap is looked at
    assert P(b"bad\n", 4, 0) == ([], dash.OK)
    first = b"WR 0x12 5".ljust(19)                                # 19 bytes, no newline: one record
    assert P(first + b"RD 0x01\n") == ([0x8000 | 0x1200 | 5, 0x0100], dash.OK)
    assert P(first + b"\n") == ([0x8000 | 0x1200 | 5], dash.EPARSE)  # the 20th byte is an empty record


def _tree(tmp_path, names, num_procs, sizes):
    dirs = []
    rng = np.random.default_rng(5)
    for k, name in enumerate(names):
        d = tmp_path / name
        d.mkdir()
        for t in range(num_procs):
            n = sizes[(k * num_procs + t) % len(sizes)]
            (d / f"core_{t}.txt").write_bytes(bytes(rng.integers(1, 127, n, dtype=np.uint8)))
        dirs.append(d)
    return dirs


def test_read_dirs_text_layout(dash, tmp_path):
    N, M = 4, 8  # a file's share: 19 * 8 = 152 bytes
    dirs = _tree(tmp_path, ["a", "b", "c"], N, [0, 1, 15, 16, 17, 151, 152, 153, 400])
    rc, need, slab, off, ln = dash.read_dirs_text(dirs, N, M)
    assert rc == dash.OK and len(off) == len(ln) == 12
    end = 0
    for k, d in enumerate(dirs):
        for t in range(N):
            f = k * N + t
            want = (d / f"core_{t}.txt").read_bytes()[:19 * M]
            assert off[f] % 16 == 0 and off[f] >= end and off[f] - end < 16
            assert slab[int(off[f]):int(off[f]) + int(ln[f])] == want
            end = int(off[f]) + int(ln[f])
    assert need == end                              # exact: the last file's last byte
    rc2, need2, _, _, _ = dash.read_dirs_text(dirs, N, M, cap=need - 1)
    assert rc2 == dash.EINVAL and need2 == need     # one byte short: refused, and the need restated
    rc3, need3, slab3, _, _ = dash.read_dirs_text(dirs, N, M, cap=need + 7)
    assert rc3 == dash.OK and need3 == need and slab3[:need] == slab


def test_read_dirs_text_golden_and_missing(dash, tmp_path, capfd):
    rc, need, slab, off, ln = dash.read_dirs_text([GOLDEN / "sample"], 4, 32)
    assert rc == dash.OK
    for t in range(4):
        data = slab[int(off[t]):int(off[t]) + int(ln[t])]
        assert data == (GOLDEN / "sample" / f"core_{t}.txt").read_bytes()[:19 * 32]
        words, prc = dash.parse_core_text(data, 4, 32)
        assert prc == dash.OK and words.tolist() == dash.parse_core_file(GOLDEN / "sample" / f"core_{t}.txt").tolist()
    dirs = _tree(tmp_path, ["x", "y"], 4, [40])
    (dirs[1] / "core_2.txt").unlink()
    capfd.readouterr()
    rc, _, _, _, _ = dash.read_dirs_text(dirs, 4, 32)
    assert rc == dash.EIO
    assert f"Error: count not open file {dirs[1]}/core_2.txt" in capfd.readouterr().err
