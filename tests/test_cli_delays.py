"""cache_simulator --delays and --explore-delays (GPU): one delay word run end to end, the outcome lines of
a delay space, and a printed witness pasted back into --delays."""
import shutil
import subprocess

import pytest

import delay_ref as dr
import oracle_ctypes as oc
from oracle_ctypes import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture
def cli(dash, tmp_path):
    (tmp_path / "tests").mkdir()
    for t in ("test_3", "test_4"):
        shutil.copytree(GOLDEN / t, tmp_path / "tests" / t)
    exe = dash.PKG / "cache_simulator"

    def run(*args, ok=True):
        p = subprocess.run([str(exe), *args], cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert (p.returncode == 0) == ok, p.stderr
        # (a directory run prints the reference's "Processor <n> initialized" lines first)
        return [ln for ln in p.stdout.splitlines() if not ln.endswith(" initialized")] if ok else p.stderr
    run.dir = tmp_path
    return run


def dumps(d):
    return [(d / f"core_{n}_output.txt").read_bytes() for n in range(4)]


def test_delays_writes_run_4(dash, cli):
    """The recorded two-delay witness of test_4's accepted run_4, as --delays takes it."""
    hit = [o for o in dr.recorded("test_4") if o["digest"] == dr.accepted_digest("test_4", "run_4")]
    word = dr.word_at(dr.lockstep_rounds("test_4"), 4, 7, 2, hit[0]["seed"])
    spec = dash.delay_format(word)
    assert spec.count(",") == 1 and dash.delay_pack(
        [tuple(int(x) for x in s.replace("@", "+").split("+")) for s in spec.split(",")]) == word
    assert cli("test_4", "--delays", spec) == []
    assert dumps(cli.dir) == dumps(GOLDEN / "test_4" / "run_4")
    # "-" is lockstep: run_1
    assert cli("test_4", "--delays", "-") == []
    assert dumps(cli.dir) == dumps(GOLDEN / "test_4" / "run_1")
    # --coherence and --debug-msg work as under --schedule
    lines = cli("test_4", "--delays", spec, "--coherence", "--debug-msg")
    res, log = dr.run_word(*dr.golden("test_4"), word, log=True, log_msgs=True)
    want = [ln for ln in log.splitlines() if " msg from: " in ln]
    assert lines[:len(want)] == want and len(lines) == len(want) + 1 and "coherence" in lines[-1]
    for bad in ("4@", "0@1+3", "8@0+1", "0@1023+1", "0@0+256", "0@0+1,", "0@0+1,0@0+1,0@0+1,0@0+1,0@0+1"):
        assert "--delays" in cli("test_4", "--delays", bad, ok=False)
    assert "--schedule" in cli("test_4", "--delays", spec, "--schedule", "5", ok=False)


@pytest.mark.parametrize("flags", [[], ["--coherence"]])
def test_explore_delays_lines_and_paste(dash, cli, flags):
    """--explore-delays 1 at the defaults (R = the lockstep rounds, E = 7): one line per outcome of the
    oracle's list, and every printed witness, pasted into --delays, writes that outcome's state."""
    for test in ("test_3", "test_4"):
        want = dr.golden_list(test, 1)
        lines = cli(test, "--explore-delays", "1", *flags)
        R = dr.lockstep_rounds(test)
        assert lines == [
            f"{o['digest']:016x} {o['count']} {o['seed']} {o['rounds']} {o['errors']:x}"
            + (f" {o['bits']:x}" if flags else "") + " " + (dash.delay_format(dr.word_at(R, 4, 7, 1, o["seed"])) or "-")
            for o in want]
        assert lines == cli(test, "--explore-delays", "1", "--delay-starts", str(R), "--delay-lens", "7", *flags)
        clean = [ln for ln in lines if ln.split()[4] == "0"]  # (a run with error bits exits 2)
        assert len(clean) >= 2
        for ln in clean[:3]:
            f = ln.split()
            cli(test, "--delays", f[-1], "-o", ".")
            texts = [(cli.dir / f"core_{n}_output.txt").read_text() for n in range(4)]
            assert oc.dumps_digest(texts) == int(f[0], 16), ln
    assert "--explore-delays" in cli("test_3", "--explore-delays", "5", ok=False)


def test_explore_delays_sources(dash, cli):
    (cli.dir / "more.txt").write_text("test_4\n")
    own = {t: cli(t, "--explore-delays", "1", "--delay-starts", "20", "--delay-lens", "3") for t in ("test_3", "test_4")}
    both = cli("test_3", "--explore-delays", "1", "--delay-starts", "20", "--delay-lens", "3", "--sources", "more.txt")
    K = dr.count(20, 4, 3, 1)
    assert both[:-2] == [f"0 {ln}" for ln in own["test_3"]] + [f"1 {ln}" for ln in own["test_4"]]
    assert [ln.split(" incoherent=")[0] for ln in both[-2:]] == [
        f"source {g} {t} outcomes={len(own[t])} schedules={K}" for g, t in enumerate(("test_3", "test_4"))]
