"""csrc/dash_text.c under gcc's AddressSanitizer + UBSan (CPU only, a stand-alone
program run as a child process: tools/text_sanitize.c). The in-memory parser
reads exact-size heap copies of the corpus files, so a one-byte over-read is a
report; the directory reader fills a buffer of exactly the measured size."""
import os
import pathlib
import shutil
import subprocess

import pytest

import text_corpus as tc

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = ROOT / "ue22cs343bb1-openmp-assignment_amd" / "csrc"


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_text_code_under_asan_ubsan(tmp_path):
    exe = tmp_path / "text_sanitize"
    cmd = ["gcc", "-O1", "-g", "-std=c11", "-D_POSIX_C_SOURCE=200809L",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-I", str(ROOT / "include"), "-I", str(CSRC), str(ROOT / "tools" / "text_sanitize.c"),
           str(CSRC / "dash_text.c"), str(CSRC / "dash_host.c"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    corpus = tmp_path / "corpus"
    corpus.mkdir()
    for i, data in enumerate(tc.corpus()):
        (corpus / f"f{i}.txt").write_bytes(data)
    scratch = tmp_path / "scratch"
    scratch.mkdir()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([str(exe), str(corpus), str(len(tc.corpus())), str(scratch)], capture_output=True, text=True,
                       timeout=600, env=env)
    assert p.returncode == 0, (p.stdout + p.stderr)[-4000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    assert "text sanitizer run clean" in p.stdout
