#!/usr/bin/env python3
"""What dash_shrink_many costs against the route a user had before it existed, in one process.

One handle of --systems systems x 8 nodes, CACHE_SIZE 4, lockstep (created without a schedule seed), its
batch generated on the device (uniform RD/WR). The jobs are the first J systems that end incoherent with no
error bit, each under the goal "the lowest bit of its own record, no error bit". Two inputs:

  long   64 sources of 8 x 4,096 instructions (profiles/shrink.json's input, 64 of them)
  short  4,096 sources of 8 x 64 instructions

(a) dash_shrink_many over all jobs: a host clock around the call (it returns with the stream synchronised),
    and its report: sim_ms / gen_ms / select_ms (device events), lock-step rounds, dash_run calls, variants.
(b) the yardstick, the route without it: a loop of dash_shrink (the same engine, one job per call) over the
    same jobs on the same handle, the host clock around each call, summed. A call overwrites the batch, so
    the generator puts the sources back before every call of either route; that time is kept apart
    (restore_s) and is in neither total.
The two routes alternate, --reps rounds (fewer when --budget-s runs out; reps_done says how many), medians;
every round asserts identical steps, traces and lengths, job by job. Nothing is gated: the figures go to
--out (profiles/shrink_many.json) with the box probe. A gain is stated in spreads: (median of (b) - median
of (a)) over the wider of the two routes' max - min."""
import argparse
import json
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from __graft_entry__ import load_package  # noqa: E402

GEN_SEED = 0x5EED
INPUTS = {"long": (64, 4096), "short": (4096, 64)}  # name: (jobs, instructions per node)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def as_steps(steps):
    return [tuple(int(x) for x in s) for s in steps]


def measure(dash, name, S, reps, budget_s, max_rounds, device):
    J, L = INPUTS[name]
    N, CS = 8, 4
    rec = {"workload": f"the first {J} incoherent, error-free systems of {S} generated systems x {N} nodes x {L} uniform "
                       f"RD/WR per node, CACHE_SIZE {CS}, lockstep, on a handle of {S} systems (DASH_KEEP_STATE)",
           "jobs": J, "len": L, "systems": S, "reps_asked": reps}
    with dash.Engine(S, num_procs=N, cache_size=CS, max_instr=L, device=device, keep_state=True) as eng:
        restore = lambda: eng.generate(GEN_SEED, L, kind=dash.GEN_UNIFORM)
        restore()
        eng.run()
        eng.check_coherence()
        coh, err = eng.read_coherence(), eng.read_results()[2]
        srcs = np.flatnonzero((coh["bits"] != 0) & (err == 0))[:J]
        if len(srcs) < J:
            print(json.dumps({"shrink_many_row": "TOO FEW INCOHERENT SYSTEMS", "input": name, "found": len(srcs)}))
            return None
        jobs = [(int(s), 0, int(coh["bits"][s]) & -int(coh["bits"][s]), 0, 0xFFFFFFFF) for s in srcs]
        # one untimed call of each route: code objects loaded, buffers allocated; the rounds there are
        restore()
        first = eng.shrink_many(jobs, cap=max_rounds)
        if int(first["results"]["rounds"].max()) > max_rounds or first["report"]["unmet"]:
            print(json.dumps({"shrink_many_row": "TOO MANY ROUNDS OR AN UNMET JOB", "input": name,
                              "rounds": int(first["results"]["rounds"].max()), "unmet": first["report"]["unmet"]}))
            return None
        steps_a = [as_steps(s) for s in first["steps"]]
        restore()
        eng.shrink(jobs[0][0], jobs[0][2], cap=max_rounds)
        many_s, loop_s, restore_s, reports, loop_reports = [], [], [], [], []
        t_start = time.perf_counter()
        for _ in range(reps):
            if many_s and budget_s and time.perf_counter() - t_start > budget_s:
                break
            t0 = time.perf_counter()
            restore()
            t_restore = time.perf_counter() - t0
            t0 = time.perf_counter()
            got = eng.shrink_many(jobs, cap=max_rounds)
            many_s.append(time.perf_counter() - t0)
            reports.append(got["report"])
            assert [as_steps(s) for s in got["steps"]] == steps_a
            assert np.array_equal(got["trace"], first["trace"]) and np.array_equal(got["lens"], first["lens"])
            t_loop, sums = 0.0, {"passes": 0, "variants": 0, "sim_ms": 0.0, "gen_ms": 0.0, "select_ms": 0.0}
            for i, (src, _seed, bit, _ea, _en) in enumerate(jobs):
                t0 = time.perf_counter()
                restore()
                t_restore += time.perf_counter() - t0
                t0 = time.perf_counter()
                alone = eng.shrink(src, bit, cap=max_rounds)
                t_loop += time.perf_counter() - t0
                assert as_steps(alone["steps"]) == steps_a[i], "the two routes disagree"
                assert np.array_equal(alone["trace"], got["trace"][i]) and np.array_equal(alone["lens"], got["lens"][i])
                for f in sums:
                    sums[f] += alone["report"][f]
            loop_s.append(t_loop)
            restore_s.append(t_restore)
            loop_reports.append(sums)
            print(json.dumps({"input": name, "shrink_many_s": many_s[-1], "shrink_loop_s": loop_s[-1]}), flush=True)
    rep = reports[0]
    med = lambda rs, f: spread([r[f] for r in rs])
    rounds = first["results"]["rounds"]
    gain = statistics.median(loop_s) - statistics.median(many_s)
    width = max(max(many_s) - min(many_s), max(loop_s) - min(loop_s))
    rec["input"] = {"first_source": jobs[0][0], "last_source": jobs[-1][0], "instr_before": rep["instr_before"],
                    "instr_after": rep["instr_after"], "job_rounds": {"min": int(rounds.min()), "max": int(rounds.max()),
                                                                      "mean": float(rounds.mean())}}
    rec["dash_shrink_many"] = {"what": "host clock around dash_shrink_many (returns synchronised); report fields by device events",
                               "total_s": spread(many_s), "sim_ms": med(reports, "sim_ms"), "gen_ms": med(reports, "gen_ms"),
                               "select_ms": med(reports, "select_ms"), "lockstep_rounds": rep["rounds"],
                               "dash_run_calls": rep["passes"], "variants": rep["variants"],
                               "host_bytes_read_per_round": 8}
    rec["dash_shrink_loop"] = {"what": "a loop of dash_shrink over the same jobs on the same handle: host clock around each "
                                       "call, summed; report fields summed over the calls",
                               "total_s": spread(loop_s), "sim_ms": med(loop_reports, "sim_ms"),
                               "gen_ms": med(loop_reports, "gen_ms"), "select_ms": med(loop_reports, "select_ms"),
                               "dash_run_calls": loop_reports[0]["passes"], "variants": loop_reports[0]["variants"]}
    rec["restore_s"] = {"what": "the generator putting the sources back before every call of either route; in neither total",
                        **spread(restore_s)}
    rec["reps_done"] = len(many_s)
    rec["results_identical_in_every_round"] = True
    rec["loop_over_many"] = {"median": statistics.median(loop_s) / statistics.median(many_s),
                             "per_round": spread([b / a for a, b in zip(many_s, loop_s)])}
    rec["gain_s"] = gain
    rec["spread_s"] = width
    rec["gain_in_spreads"] = gain / width if width else None
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--systems", type=int, default=65536)
    ap.add_argument("--inputs", default="long,short")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-rounds", type=int, default=400)
    ap.add_argument("--budget-s", type=float, default=0, help="per input: start no further alternating round after this "
                                                             "many seconds of them (0: all --reps)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "shrink_many.json"))
    args = ap.parse_args()
    dash = load_package()
    committed = ROOT / "profiles" / "shrink_many.json"  # inputs measured in an earlier call stay in the record
    out = json.loads(committed.read_text()) if committed.exists() else {"tool": "tools/shrink_many_row.py", "inputs": {}}
    out["box"] = dash.probe_box(args.device)
    for name in args.inputs.split(","):
        rec = measure(dash, name, args.systems, args.reps, args.budget_s, args.max_rounds, args.device)
        if rec is None:
            return 1
        rec["box"] = out["box"]
        out["inputs"][name] = rec
        print(json.dumps({"shrink_many_row": "ok", "input": name, "shrink_many_s": rec["dash_shrink_many"]["total_s"]["median"],
                          "shrink_loop_s": rec["dash_shrink_loop"]["total_s"]["median"],
                          "loop_over_many": rec["loop_over_many"]["median"], "gain_in_spreads": rec["gain_in_spreads"]}),
              flush=True)
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
