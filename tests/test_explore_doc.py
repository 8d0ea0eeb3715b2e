"""INTEGRATION.md §2c (which outcomes can this directory reach) is code a maintainer copies: it
compiles against include/dash.h with plain gcc, and on the GPU it runs from the repository's
tests/golden/reference/test_4 and prints what the oracle finds for the same seeds."""
import pathlib
import re
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
PKG = ROOT / "ue22cs343bb1-openmp-assignment_amd"
DOC = (ROOT / "INTEGRATION.md").read_text()
GOLDEN = ROOT / "tests" / "golden" / "reference"


def snippet():
    body = next(b for b in re.findall(r"```c\n(.*?)```", DOC, flags=re.S) if "dash_explore" in b)
    return ("#include <stdint.h>\n#include <stdio.h>\n#include <stdlib.h>\n#include \"dash.h\"\n"
            "int main(void) {\n" + body + "    (void)sched;\n    free(packed);\n    free(lens);\n"
            "    dash_destroy(h);\n    return 0;\n}\n")


def build(tmp_path, link):
    src = tmp_path / "explore.c"
    src.write_text(snippet())
    exe = tmp_path / "explore"
    cmd = ["gcc", "-O2", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src)]
    cmd += ["-o", str(exe), f"-L{PKG}", "-ldash", f"-Wl,-rpath,{PKG}"] if link else ["-c", "-o", str(tmp_path / "explore.o")]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def test_explore_snippet_compiles(tmp_path):
    assert "dash_seed_schedule" in snippet() and "dash_load_traces" in snippet()
    build(tmp_path, link=False)


@pytest.mark.gpu
def test_explore_snippet_runs(dash, tmp_path):
    import oracle_ctypes as oc
    exe = build(tmp_path, link=True)
    (tmp_path / "tests").mkdir()
    shutil.copytree(GOLDEN / "test_4", tmp_path / "tests" / "test_4")
    p = subprocess.run([str(exe)], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.splitlines()
    tr, lens = oc.load_test_dir(GOLDEN / "test_4")
    lock, s87 = oc.run_system(tr, lens), oc.run_system(tr, lens, arb_seed=87)
    assert lines[0].startswith(f"{lock.digest:016x} reached by ") and f"first by seed 0 in {lock.rounds} rounds" in lines[0]
    assert lines[1].startswith(f"{s87.digest:016x} reached by ") and f"first by seed 87 in {s87.rounds} rounds" in lines[1]
    assert sum(int(re.search(r"reached by (\d+) seeds", ln)[1]) for ln in lines) == 1 << 20
