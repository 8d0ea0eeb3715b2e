"""The adequacy corpus (tests/golden/adequacy/, tests/adequacy.py) on the CPU: the inputs that
tests/test_gpu_adequacy.py runs through every kernel class would catch a subtly wrong kernel.

For every node count of the fixture and every CACHE_SIZE class (the five specialised kernels and
the generic cs_lut path below and above 8), every oracle mutant -- one deviation of one handler
each: 13 misreadings of the reference, 19 slips of single terms of the kernel's mask algebra --
is told apart from the checker by at least 3 systems of the corpus run all-lockstep (what the
MODE 0 and MODE 2 kernels see) and by at least 3 under the corpus's own schedule seeds (MODE 1
and 3), and by at least one walk of the micro-step section at CACHE_SIZE 1, 4 and 3 (MODE 4). 3
is a condition, not a measurement: one coincidence must not carry a protocol state.

At N >= 3 there are no exemptions. At N = 2 a cell may be listed in the fixture's `exempt` with the
number of candidates searched (at least 50,000) and found; the found ones must be in the corpus.
At N = 1 every message is a self-message; the generated batch of adequacy.n1_batch() is checked
for the one mutant of issue_instruction that a single node can reach (N1_MUTANTS).

This shows that the inputs would catch these deviations in each kernel class. It does not show
that no other deviation exists.
"""
import functools
import importlib.util

import numpy as np
import pytest

import adequacy as ad
import oracle_ctypes as oc

_spec = importlib.util.spec_from_file_location("make_adequacy_corpus",
                                               oc.ROOT / "tests" / "golden" / "make_adequacy_corpus.py")
mk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mk)

EVALS = mk.EVALS
# of adequacy.ISSUE_SIDE (13, 24, 25, 30), what one node alone can reach: m13 only. The others need
# two nodes and are skipped at N = 1 -- a reply's fill always follows the node's own WR (instr.value
# is that WR's, m24), no second sharer makes a line SHARED (m25), and a line goes INVALID only
# between a WRITEBACK_INV and the FLUSH_INVACK that refills it in the same round (m30). 51,200
# one-node candidates of adequacy.candidates(1, .) tell none of the three apart at any CACHE_SIZE.
N1_MUTANTS = (13,)


@functools.lru_cache(maxsize=None)
def fixture(N):
    return ad.load_fixture(N)


def exempt_cell(N, k, CS, ev):
    for e in fixture(N)["exempt"]:
        if (e["mutant"], e["cache_size"], e["evaluation"]) == (k, CS, ev):
            return e
    return None


@pytest.mark.parametrize("N", ad.NODE_COUNTS)
def test_fixture_is_what_the_generator_writes(N):
    fx = fixture(N)
    raw = fx["raw"]
    text = (ad.FIXTURE_DIR / f"n{N}.json").read_text()
    assert len(text) < 200_000
    assert 1 <= len(raw["systems"]) <= ad.MAX_SYSTEMS and 1 <= len(raw["micro"]) <= ad.MAX_MICRO
    assert fx["lens"].max() <= ad.MAX_LEN and raw["num_procs"] == N
    assert (fx["seeds"] != 0).all() and (fx["seeds"] >> np.uint64(32)).any()  # 64-bit schedule seeds
    again = mk.fixture_from_ids(N, [s["cand"] for s in raw["systems"]], [s["cand"] for s in raw["micro"]],
                                raw.get("exempt", []), raw["candidates_searched"])
    assert mk.dumps(again) == text
    if N >= 3:
        assert "exempt" not in raw
    for e in fx["exempt"]:
        assert e["searched"] >= 50_000 and e["found"] < ad.MIN_KILLS and len(e["systems"]) == e["found"]
        assert e["mutant"] in ad.MUTANTS and e["evaluation"] in EVALS
        assert e["cache_size"] in ad.CACHE_SIZES


@pytest.mark.parametrize("CS", ad.CACHE_SIZES)
@pytest.mark.parametrize("N", ad.NODE_COUNTS)
def test_every_mutant_is_told_apart_in_the_round_model(N, CS):
    fx = fixture(N)
    for ev, seeds in zip(EVALS, (None, fx["seeds"])):
        base = ad.run_many(ad.lib(0), fx["packed"], fx["lens"], N, CS, seeds)
        assert base[1].max() <= 16, "a system leaves the first queue tier"
        assert not (base[2] & ad.BAD_ERRORS).any()
        for k in ad.MUTANTS:
            dead = np.flatnonzero(ad.kills(ad.lib(k), fx["packed"], fx["lens"], N, CS, seeds, base)).tolist()
            e = exempt_cell(N, k, CS, ev)
            if e is not None:  # every candidate the search found is in the corpus, and kills
                assert dead == e["systems"], (k, ev)
            else:
                assert len(dead) >= ad.MIN_KILLS, f"m{k} ({ad.MUTANTS[k]}): {ev}, told apart by systems {dead}"


@pytest.mark.parametrize("N", ad.NODE_COUNTS)
def test_every_mutant_is_told_apart_by_a_micro_step_walk(N):
    fx = fixture(N)
    for CS in ad.MICRO_CS:
        dead = {k: 0 for k in ad.MUTANTS}
        for tr, lens, wseed, weights in fx["micro"]:
            w = ad.walk(tr, lens, N, CS, wseed, weights)
            assert w is not None, "a queue of the micro-step model overflowed"
            out, steps = w
            assert not out.errors & (oc.ERR_ROUNDCAP | oc.ERR_STUCK)
            for k in ad.MUTANTS:
                dead[k] += ad.micro_kills(ad.lib(k), tr, lens, N, CS, steps)
        short = [k for k, n in dead.items() if n < 1 and exempt_cell(N, k, CS, "micro") is None]
        assert not short, (CS, short)


@pytest.mark.parametrize("CS", ad.CACHE_SIZES)
def test_one_node_batch_tells_the_issue_side_mutants_apart(CS):
    packed, lens, seeds = ad.n1_batch()
    for sd in (None, seeds):
        base = ad.run_many(ad.lib(0), packed, lens, 1, CS, sd)
        assert base[1].max() <= 16 and not (base[2] & ad.BAD_ERRORS).any()
        for k in N1_MUTANTS:
            assert ad.kills(ad.lib(k), packed, lens, 1, CS, sd, base).sum() >= ad.MIN_KILLS, k


def test_mutant_table():
    """1..13 are ref_pin's (unchanged), the kernel-shaped ones continue at 14; at least 12 of the
    issue's 19 candidates remain, and the oracle's Makefile builds exactly this list."""
    import re
    import ref_pin
    assert {k: ad.MUTANTS[k] for k in ref_pin.MUTANTS} == ref_pin.MUTANTS and sorted(ref_pin.MUTANTS) == list(range(1, 14))
    new = sorted(k for k in ad.MUTANTS if k >= 14)
    assert len(new) >= 12 and not set(new) & set(ad.EQUIVALENT) and set(new) | set(ad.EQUIVALENT) == set(range(14, 33))
    mkf = (oc.ORACLE_DIR / "Makefile").read_text().replace("\\\n", " ")
    assert [int(x) for x in re.search(r"^MUTANTS := (.*)$", mkf, re.M)[1].split()] == sorted(ad.MUTANTS)
    assert set(ad.ISSUE_SIDE) <= set(ad.MUTANTS)
