"""The host trace-text parsers against the C library's sscanf (CPU only).

dash_parse_core_file and dash_parse_core_text restate fgets(line, 20) + sscanf by hand;
test_text_parse.py pins them on each other. Here both are held to tests/sscanf_ref.py, which
calls the library's sscanf with the reference's two formats, and the reference binary itself
is run on the classes where a hand-written scanner and the library once parted (DESIGN.md
§5.3). No expected value below is written by hand: every one is the twin's.

The second corpus and the enumeration (text_corpus.py) are judged by the twin alone first, so a
generator that stops producing a class fails here instead of letting the comparison go quiet.
"""
import random
import re
import subprocess

import pytest

import oracle_ctypes as oc
import ref_pin
import sscanf_ref as twin
import text_corpus as tc


@pytest.fixture(scope="module")
def on_disk(tmp_path_factory):
    """Both corpora as files, written once: (data, path) pairs."""
    root = tmp_path_factory.mktemp("sscanf")
    out = []
    for name, files in (("a", tc.corpus()), ("b", tc.scanf_corpus())):
        for i, data in enumerate(files):
            p = root / f"{name}{i}.txt"
            p.write_bytes(data)
            out.append((data, p))
    return out


def _reached(data, num_procs, max_instr):
    """The records the twin looks at: the accepted ones and the one that fails."""
    words, _ = twin.parse_core_text(data, num_procs, max_instr)
    return [rec for i, rec in enumerate(twin.records(data)) if i <= len(words) and i < max_instr]


def test_second_corpus_covers_every_class():
    files = tc.scanf_corpus()
    assert len(files) == tc.SCANF_FILES and all(len(d) <= 19 * 64 for d in files)
    assert twin.OK == 0 and (twin.EPARSE, twin.EADDR) == (-3, -4)
    ok = eparse = eaddr = capped = 0
    holds = dict.fromkeys(tc.CLASSES, 0)        # files with a record of the class, judged as the class says
    deviating = dict.fromkeys(tc.DEVIATIONS, 0)  # records of a deviation class that the library accepts
    for data in files:
        words, rc = twin.parse_core_text(data, 4, 32)
        _, rc_full = twin.parse_core_text(data, 4, 4096)
        ok += rc == twin.OK
        eparse += rc == twin.EPARSE
        eaddr += rc == twin.EADDR
        capped += rc == twin.OK and len(words) == 32 and rc_full != twin.OK
        recs = _reached(data, 4, 32)
        for name, (pat, accepted) in tc.CLASSES.items():
            holds[name] += any(re.match(pat, r) and twin.accepts(r) == accepted for r in recs)
        for name, pat in tc.DEVIATIONS.items():
            deviating[name] += sum(bool(re.match(pat, r)) and twin.accepts(r) for r in recs)
    assert min(ok, eparse, eaddr, capped) >= 3, (ok, eparse, eaddr, capped)
    assert all(n >= 3 for n in holds.values()), holds
    assert all(n >= 3 for n in deviating.values()), deviating


def test_enumeration_covers_the_deviations():
    recs, exhaustive = tc.enumeration()
    assert exhaustive == 2 * sum(len(tc.ALPHABET) ** n for n in range(5)) and len(set(recs)) == len(recs)
    assert len(recs) > exhaustive + 19000         # the draws are long enough to be distinct
    for name, pat in tc.DEVIATIONS.items():
        if name != "saturation":                  # 17 digits: longer than any record drawn here
            assert sum(bool(re.match(pat, r)) and twin.accepts(r) for r in recs) >= 3, name


@pytest.mark.parametrize("num_procs", [3, 4, 8])
@pytest.mark.parametrize("max_instr", [0, 1, 32])
def test_parsers_equal_sscanf(dash, on_disk, num_procs, max_instr):
    assert (dash.OK, dash.EPARSE, dash.EADDR) == (twin.OK, twin.EPARSE, twin.EADDR)
    bad = []
    for data, path in on_disk:
        want, want_rc = twin.parse_core_text(data, num_procs, max_instr)
        for name, (got, rc) in (("text", dash.parse_core_text(data, num_procs, max_instr)),
                                ("file", tc.parse_file(dash, path, num_procs, max_instr))):
            if rc != want_rc or got.tolist() != want.tolist():
                bad.append((name, path.name, data, (got.tolist(), rc), (want.tolist(), want_rc)))
    assert not bad, (len(bad), bad[:3])


def test_enumeration_equals_sscanf(dash, tmp_path):
    """Each record of the enumeration as a file of its own, at num_procs 8."""
    recs, _ = tc.enumeration()
    path = tmp_path / "rec.txt"
    bad = []
    for rec in recs:
        want, want_rc = twin.parse_core_text(rec, 8, 32)
        path.write_bytes(rec)
        for name, (got, rc) in (("text", dash.parse_core_text(rec, 8, 32)), ("file", tc.parse_file(dash, path, 8, 32))):
            if rc != want_rc or got.tolist() != want.tolist():
                bad.append((name, rec, (got.tolist(), rc), (want.tolist(), want_rc)))
    assert not bad, (len(bad), bad[:5])


# ---------------------------------------------------------------- the reference itself

PIN = ref_pin.pin_exe(4)  # the reference at its own NUM_PROCS 4 / MAX_INSTR_NUM 32, DEBUG_INSTR, terminating


def self_homed_dir(seed):
    """Four files of up to 32 records from the new classes, all accepted by the twin and every
    address homed on the file's own node: every message is a self-message, so the run does not
    depend on the schedule."""
    rng = random.Random(seed)
    files = []
    for node in range(4):
        recs = []
        for _ in range(rng.randrange(20, 33)):
            while True:
                r = tc.scanf_record(rng, node=node)
                got = twin.scan_record((r + "\n").encode("latin-1")[:19])
                if got is not None and got[1] >> 4 == node:
                    break
            recs.append(r)
        files.append(tc._join(rng, recs).encode("latin-1"))
    return files


@pytest.mark.skipif(not PIN.exists(), reason="reference pin binary not built")
@pytest.mark.parametrize("seed", range(4))
def test_reference_issues_what_the_parser_returns(dash, tmp_path, seed):
    files = self_homed_dir(0x5EED + seed)
    d = tmp_path / "tests" / "t"
    d.mkdir(parents=True)
    for n, data in enumerate(files):
        (d / f"core_{n}.txt").write_bytes(data)
        words, rc = twin.parse_core_text(data, 4, 32)
        assert rc == twin.OK and 20 <= len(words) <= 32     # only records the library accepts
    devs = [sum(bool(re.match(pat, r)) for data in files for r in twin.records(data)) for pat in tc.DEVIATIONS.values()]
    assert all(n >= 1 for n in devs[:3]), devs              # a saturated address is homed on no node of 4
    p = subprocess.run(["timeout", "20", str(PIN), "t"], cwd=tmp_path, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    _, instr = oc.parse_logs(p.stdout, 4)
    for n in range(4):
        words = dash.parse_core_file(d / f"core_{n}.txt", 4, 32)
        assert instr[n] == words.tolist(), n
