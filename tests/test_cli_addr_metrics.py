"""`cache_simulator <dir> --addr-metrics`: one stdout line per touched address, equal to the Engine's
records for the same directory, after dumps that are still byte-equal to the goldens; and the usage
text names the flag."""
import shutil
import subprocess

import pytest

import addr_metrics_ref as ar
import oracle_ctypes as oc
from oracle_ctypes import GOLDEN

CLASS_NAMES = ("untouched", "private", "read_shared", "one_writer", "multi_writer")


def test_usage_names_the_flag(dash):
    p = subprocess.run([str(dash.PKG / "cache_simulator")], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "--addr-metrics" in p.stderr and "--metrics" in p.stderr


@pytest.mark.gpu
def test_cli_addr_metrics(dash, tmp_path):
    exe = dash.PKG / "cache_simulator"
    (tmp_path / "tests").mkdir()
    shutil.copytree(GOLDEN / "sample", tmp_path / "tests" / "sample")
    p = subprocess.run([str(exe), "sample", "--addr-metrics"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert [(tmp_path / f"core_{n}_output.txt").read_bytes() for n in range(4)] == \
        [(GOLDEN / "sample" / f"core_{n}_output.txt").read_bytes() for n in range(4)]
    lines = p.stdout.splitlines()
    assert lines[:4] == [f"Processor {n} initialized" for n in range(4)]
    tr, lens = oc.load_test_dir(GOLDEN / "sample")
    with dash.Engine(1, num_procs=4, cache_size=4, max_instr=32, trace_events=1024) as eng:
        eng.load_traces(tr[None], lens[None])
        eng.run()
        eng.compute_addr_metrics()
        rec = eng.read_addr_metrics()[0][0]
    want = {a: m for a, m in enumerate(rec) if dash.addr_class(m) != dash.ADDR_UNTOUCHED}
    assert want and len(lines) == 4 + len(want)
    got_addrs = []
    for line in lines[4:]:
        words = line.split()
        assert words[0] == "addr" and words[1].startswith("0x") and len(words[1]) == 4
        a = int(words[1], 16)
        got_addrs.append(a)
        got = dict(w.split("=") for w in words[2:])
        m = want[a]
        assert got.pop("class") == CLASS_NAMES[dash.addr_class(m)]
        nodes = int(m["nodes"])
        sets = {k: got.pop(k) for k in ("readers", "writers", "invalidated")}
        assert sets == {"readers": f"0x{nodes & 0xFF:02X}", "writers": f"0x{(nodes >> 8) & 0xFF:02X}",
                        "invalidated": f"0x{(nodes >> 16) & 0xFF:02X}"}
        assert list(got) == list(ar.SUM_FIELDS)  # the fields in the record's order
        assert {k: int(v) for k, v in got.items()} == {f: int(m[f]) for f in ar.SUM_FIELDS}, a
    assert got_addrs == sorted(want)  # ascending, the touched addresses exactly
    # together with --metrics: the node lines first, then the same address lines
    both = subprocess.run([str(exe), "sample", "--metrics", "--addr-metrics"], cwd=tmp_path, capture_output=True,
                          text=True, timeout=120)
    assert both.returncode == 0, both.stderr
    out = both.stdout.splitlines()
    assert [ln.split()[0] for ln in out[4:8]] == ["metrics"] * 4 and out[8:] == lines[4:]
