#!/usr/bin/env python3
"""Writes tests/golden/delay_outcomes.json: for test_3 and test_4, the outcomes of every schedule within
two delays of lockstep (start rounds 0 .. lockstep rounds - 1, lengths 1 .. 64) as the CPU oracle runs
them under each schedule's explicit round table -- tests/delay_ref.py states the space without libdash.
Per outcome: digest, errors, count, the lowest schedule index that reached it, that witness's rounds and
the coherence record of its final state (tests/coherence_ref.py). About 1.4 million oracle runs, a few
minutes on one core. Run from the repository root after `make -C oracle`."""
import json
import pathlib
import sys

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import delay_ref as dr  # noqa: E402


def main():
    out = {}
    for test in ("test_3", "test_4"):
        R = dr.lockstep_rounds(test)
        outcomes = dr.oracle_list(*dr.golden(test), R, 7, 2)
        out[test] = {"starts": R, "lens": 7, "max_delays": 2, "schedules": dr.count(R, 4, 7, 2),
                     "outcomes": [{**o, "digest": f"{o['digest']:016x}"} for o in outcomes]}
        print(test, out[test]["schedules"], "schedules,", len(outcomes), "outcomes", file=sys.stderr)
    dr.OUTCOMES_JSON.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
