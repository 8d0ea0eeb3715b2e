#!/usr/bin/env python3
"""What dash_explore_delays costs and finds, against the routes a user had before it existed.

Default mode, one process: tests/golden/reference/test_4 at D = 2, R = its lockstep rounds, E = 7
(980,701 schedules) on a 2^20-system handle, --reps timed calls after one untimed one; medians with their
spreads (min, max). Host clock around the calls; sim_ms and merge_ms are the call's own device-event sums
(dash_explore_totals; the fill kernel's time is part of merge_ms). Against, in the same process:
  (1) the same enumeration through the host: the words built with dash_delay_word, then
      dash_set_system_delays, dash_run, dash_read_results and a merge in numpy; the lists must be equal;
  (2) dash_explore_sources with as many seeds: how many outcomes each search finds.
--ab: the seeded kernels changed, so one line of JSON with dash_explore_sources on one source (test_4)
with 2^20 seeds on a 2^20-system handle, sim_ms and host ms over --reps calls. --pkg DIR runs it on
another build's package directory (dash.py next to its libdash.so), so that a job can alternate child
processes of the parent commit's build and this one's; --ab-parent / --ab-tree fold those lines into --out.
Everything goes to --out (profiles/explore_delays.json); the README row is printed."""
import argparse
import importlib.util
import json
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
GOLDEN = ROOT / "tests" / "golden" / "reference"
NSYS, TEST, E, D = 1 << 20, "test_4", 7, 2


def load_dash(pkg):
    spec = importlib.util.spec_from_file_location("dash_amd", pathlib.Path(pkg) / "dash.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules["dash_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def golden_engine(dash, nsys):
    import oracle_ctypes as oc
    tr, lens = oc.load_test_dir(GOLDEN / TEST)
    eng = dash.Engine(nsys, num_procs=4, cache_size=4, max_instr=32, schedule_seed=1, keep_state=True)
    packed, ln = np.zeros((nsys, 4, tr.shape[1]), np.uint16), np.zeros((nsys, 4), np.uint32)
    packed[0], ln[0] = tr, lens
    eng.load_traces(packed, ln)
    return eng


def timed(fn, reps):
    fn()
    out, ms = None, []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, ms


def ab(dash, reps):
    with golden_engine(dash, NSYS) as eng:
        sims, host = [], []
        eng.explore_sources(1, 0, NSYS)
        for _ in range(reps):
            t0 = time.perf_counter()
            outs, _, tot = eng.explore_sources(1, 0, NSYS)
            host.append((time.perf_counter() - t0) * 1e3)
            sims.append(tot["sim_ms"])
        print(json.dumps({"sim_ms": sims, "host_ms": host, "outcomes": len(outs),
                          "checksum": int(outs["digest"].sum(dtype=np.uint64))}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pkg", default=str(ROOT / "ue22cs343bb1-openmp-assignment_amd"))
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--ab-parent", nargs="*", default=[])
    ap.add_argument("--ab-tree", nargs="*", default=[])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "explore_delays.json"))
    args = ap.parse_args()
    dash = load_dash(args.pkg)
    if args.ab:
        return ab(dash, args.reps)

    import delay_ref as dr
    R = dr.lockstep_rounds(TEST)
    K = dash.delay_count(R, E, D, 4)
    rep = {"workload": f"{TEST}, D = {D}, R = {R}, E = {E}: {K} schedules on a 2^20-system handle", "schedules": K}
    with golden_engine(dash, NSYS) as eng:
        sims, merges = [], []

        def device_route():
            outs, _, tot = eng.explore_delays(1, R, E, D)
            sims.append(tot["sim_ms"])
            merges.append(tot["merge_ms"])
            return outs

        outs, ms = timed(device_route, args.reps)
        rep["explore_delays"] = {"host_ms": spread(ms), "sim_ms": spread(sims[1:]), "merge_ms": spread(merges[1:]),
                                 "outcomes": len(outs)}
        new = [tuple(int(o[f]) for f in ("digest", "errors", "count", "seed", "rounds")) for o in outs]

        # (1) the same enumeration through the host
        t0 = time.perf_counter()
        words = np.array([dash.delay_word(R, E, D, 4, i) for i in range(K)] + [dash.DELAY_LOCKSTEP] * (NSYS - K), np.uint64)
        words_ms = (time.perf_counter() - t0) * 1e3
        eng.broadcast_system(0)

        def host_route():
            eng.set_system_delays(words)
            eng.run()
            dig, rnd, err = (a[:K] for a in eng.read_results())
            keys = np.stack([dig, err.astype(np.uint64)], axis=1)
            uniq, first, counts = np.unique(keys, axis=0, return_index=True, return_counts=True)
            order = np.argsort(first)
            return [(int(uniq[k][0]), int(uniq[k][1]), int(counts[k]), int(first[k]), int(rnd[first[k]])) for k in order]

        old, ms = timed(host_route, args.reps)
        assert old == new, "the host route and dash_explore_delays disagree"
        rep["host_route"] = {"set_run_read_merge_ms": spread(ms), "words_ms_once": words_ms, "lists_equal": True}
        rep["device_over_host_route"] = rep["explore_delays"]["host_ms"]["median"] / (statistics.median(ms) + words_ms)

        # (2) as many seeds of the seeded round schedule
        (souts, _, stot), ms = timed(lambda: eng.explore_sources(1, 0, K), args.reps)
        rep["explore_sources_same_count"] = {"host_ms": spread(ms), "outcomes": len(souts)}
    for name, files in (("parent", args.ab_parent), ("tree", args.ab_tree)):
        if files:
            runs = [json.loads(pathlib.Path(f).read_text().strip().splitlines()[-1]) for f in files]
            med = [statistics.median(r["sim_ms"]) for r in runs]
            rep.setdefault("seeded_ab", {"workload": f"dash_explore_sources, {TEST}, 2^20 seeds, 2^20 systems; "
                                                     "alternating child processes, sim_ms medians per process"})
            rep["seeded_ab"][name] = {"process_medians_sim_ms": med, **spread(med), "checksums": [r["checksum"] for r in runs],
                                      "host_ms_medians": [statistics.median(r["host_ms"]) for r in runs]}
    if "seeded_ab" in rep and {"parent", "tree"} <= set(rep["seeded_ab"]):
        p, t = rep["seeded_ab"]["parent"], rep["seeded_ab"]["tree"]
        assert p["checksums"][0] == t["checksums"][0]
        rep["seeded_ab"]["tree_minus_parent_ms"] = t["median"] - p["median"]
        rep["seeded_ab"]["wider_spread_ms"] = max(p["max"] - p["min"], t["max"] - t["min"])
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(rep, indent=1) + "\n")
    x, h, s = rep["explore_delays"], rep["host_route"], rep["explore_sources_same_count"]
    print(f"| every schedule within two delays of lockstep (`dash_explore_delays`) | `test_4`, {K:,} schedules on a "
          f"2^20-system handle: **{x['host_ms']['median']:.2f} ms** ({x['sim_ms']['median']:.2f} ms of kernels + "
          f"{x['merge_ms']['median']:.2f} ms of fill and merge) against {h['set_run_read_merge_ms']['median']:.1f} ms "
          f"through the host plus {h['words_ms_once']:.0f} ms to build the words, medians of {args.reps} | "
          f"{x['outcomes']} outcomes, the list equal to the host route's and to the CPU oracle's (GPU suite); as many "
          f"seeds of the seeded round schedule reach {s['outcomes']} | `profiles/explore_delays.json` |")


if __name__ == "__main__":
    main()
