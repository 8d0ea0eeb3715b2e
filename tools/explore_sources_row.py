#!/usr/bin/env python3
"""What dash_explore_sources costs, against the route a user had before it existed.

All timings of a part are taken in one process, the routes alternating, --reps of each after one
untimed round; medians with their spreads (min, max). Host clock around the calls; sim_ms, merge_ms and
insert_ms are the new call's own device-event sums (dash_explore_totals). Loading a handle is never
inside a timed span.

(a) one source against the existing route: tests/golden/reference/test_4, 2^20 seeds from 1, on a
    65,536-system and a 2^20-system handle (the workloads of profiles/explore_micro.json), seeded round
    schedules and seeded micro-step schedules under uniform weights. Old route: dash_explore[_micro] +
    dash_check_outcomes. New: one dash_explore_sources call. The two lists must be equal.
(b) the insert kernel alone (insert_ms), 2^20 systems in one pass, from real runs that give the mixes:
    every key equal (test_1, round seeds), one key at 90 % (test_4 under micro seeds: its most frequent
    outcome and a tail of rare ones), all keys distinct (2^20 generated 8-node systems as 2^20 sources,
    one seed each). Each under the default insert (the first GROUP_KEYS keys of a wave as groups, then
    every lane for itself), DASH_TEST_INSERT_PER_LANE and DASH_TEST_INSERT_GROUPS.
(c) many sources: 4,096 generated 8-node sources x 256 seeds on a 2^20-system handle, one pass, against
    the first 64 of those sources run one by one through dash_explore + dash_check_outcomes on a
    256-system handle; the old route's time for 4,096 is the per-source median times 4,096: scaled, not
    measured. The lists of those 64 sources must be equal.
Everything goes to --out (profiles/explore_sources.json) with the box probe."""
import argparse
import json
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from __graft_entry__ import load_package  # noqa: E402

GOLDEN = ROOT / "tests" / "golden" / "reference"
OUT_FIELDS = ("digest", "count", "seed", "rounds", "errors")
COH_FIELDS = ("bits", "addrs", "first_addr", "first_bits")
GEN_SEED = 0x5EED


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def width(s):
    return s["max"] - s["min"]


def golden_engine(dash, test, nsys, flags=0, device=0):
    """A seeded 4-node handle with DASH_KEEP_STATE whose system 0 holds the golden trace set."""
    import oracle_ctypes as oc
    tr, lens = oc.load_test_dir(GOLDEN / test)
    eng = dash.Engine(nsys, num_procs=4, cache_size=4, max_instr=32, schedule_seed=1, keep_state=True, flags=flags,
                      device=device)
    packed, ln = np.zeros((nsys, 4, tr.shape[1]), np.uint16), np.zeros((nsys, 4), np.uint32)
    packed[0], ln[0] = tr, lens
    eng.load_traces(packed, ln)
    return eng


def as_rows(outs, source=None):
    keep = outs if source is None else outs[outs["source"] == source]
    return [tuple(int(o[f]) for f in OUT_FIELDS + COH_FIELDS) for o in keep]


def old_rows(outs, rec):
    return [tuple(int(o[f]) for f in OUT_FIELDS) + tuple(int(r[f]) for f in COH_FIELDS) for o, r in zip(outs, rec)]


def verdict(old, new):
    gap = old["median"] - new["median"]
    return {"new_over_old": new["median"] / old["median"], "median_gap_s": gap,
            "wider_spread_s": max(width(old), width(new)),
            "new_faster_by_more_than_the_wider_spread": bool(gap > max(width(old), width(new)))}


def part_a(dash, args):
    seeds = 1 << 20
    out = {"what": f"{seeds} schedules of test_4 (4 nodes), seeds 1 .. 2^20, one source"}
    for nsys in (65536, 1 << 20):
        for kind, weights in (("rounds", None), ("micro", dash.MICRO_UNIFORM)):
            with golden_engine(dash, "test_4", nsys, device=args.device) as old, \
                    golden_engine(dash, "test_4", nsys, device=args.device) as new:
                t_old, t_new, sim, merge, insert = [], [], [], [], []
                for k in range(args.reps + 1):
                    t0 = time.perf_counter()
                    o = old.explore(0, 1, seeds) if weights is None else old.explore_micro(0, 1, seeds)
                    rec = old.check_outcomes(0, o, weights=weights)
                    t1 = time.perf_counter()
                    outs, _, tot = new.explore_sources(1, 1, seeds, weights=weights, cap=4096)
                    t2 = time.perf_counter()
                    assert as_rows(outs) == old_rows(o, rec), (nsys, kind)
                    if k:
                        t_old.append(t1 - t0)
                        t_new.append(t2 - t1)
                        sim.append(tot["sim_ms"])
                        merge.append(tot["merge_ms"])
                        insert.append(tot["insert_ms"])
                row = {"passes": tot["passes"], "distinct_outcomes": len(outs), "lists_equal": True,
                       "old_route_s": spread(t_old), "new_call_s": spread(t_new), "new_sim_ms": spread(sim),
                       "new_merge_ms": spread(merge), "new_insert_ms": spread(insert),
                       "incoherent_schedules": tot["incoherent_schedules"]}
                row.update(verdict(row["old_route_s"], row["new_call_s"]))
                out[f"handle_{nsys}_systems_{kind}"] = row
                print(json.dumps({"a": f"{nsys} {kind}", "old_s": row["old_route_s"]["median"],
                                  "new_s": row["new_call_s"]["median"], "merge_ms": row["new_merge_ms"]["median"]}),
                      flush=True)
    return out


def part_b(dash, args):
    n = 1 << 20
    modes = (("default", 0), ("per_lane", dash.TEST_INSERT_PER_LANE), ("groups", dash.TEST_INSERT_GROUPS))
    out = {"what": f"insert_ms of one pass over {n} systems; inserts per second = {n} / median"}
    for case in ("every_key_equal", "one_key_at_90_percent", "all_keys_distinct"):
        out[case] = {}
        for mode, flag in modes:
            if case == "all_keys_distinct":
                eng = dash.Engine(n, num_procs=8, cache_size=4, max_instr=8, schedule_seed=1, keep_state=True, flags=flag,
                                  device=args.device)
                eng.generate(GEN_SEED, 8, kind=dash.GEN_UNIFORM)
                call = dict(num_sources=n, first_seed=1, seeds_per_source=1)
            else:
                eng = golden_engine(dash, "test_1" if case == "every_key_equal" else "test_4", n, flag, args.device)
                call = dict(num_sources=1, first_seed=1, seeds_per_source=n,
                            weights=None if case == "every_key_equal" else dash.MICRO_UNIFORM)
            with eng:
                ins, merge = [], []
                for k in range(args.reps + 1):
                    outs, _, tot = eng.explore_sources(cap=64, **call)
                    if k:
                        ins.append(tot["insert_ms"])
                        merge.append(tot["merge_ms"])
                top = int(outs["count"].max())
                assert tot["schedules"] == n and tot["unplaced"] == 0
            out[case][mode] = {"insert_ms": spread(ins), "merge_ms": spread(merge),
                               "inserts_per_s": n / (statistics.median(ins) * 1e-3), "distinct_keys": tot["outcomes"],
                               "largest_key_share": top / n, "table_slots": tot["table_slots"]}
            print(json.dumps({"b": case, "mode": mode, "insert_ms": statistics.median(ins),
                              "keys": tot["outcomes"]}), flush=True)
    return out


def part_c(dash, args):
    G, K, L, S, sample = 4096, 256, 16, 1 << 20, 64
    out = {"what": f"{G} generated 8-node sources (uniform, {L} instructions per node) x {K} round seeds from 0"}
    with dash.Engine(G, num_procs=8, cache_size=4, max_instr=L, device=args.device) as small:
        small.generate(GEN_SEED, L, kind=dash.GEN_UNIFORM)  # the generator is counter-based: the same systems
        packed, lens = small.read_traces()
    with dash.Engine(S, num_procs=8, cache_size=4, max_instr=L, schedule_seed=1, keep_state=True,
                     device=args.device) as big:
        t_new, sim, merge = [], [], []
        for k in range(args.reps + 1):
            big.generate(GEN_SEED, L, kind=dash.GEN_UNIFORM)  # (the call overwrites systems >= G)
            t0 = time.perf_counter()
            outs, per, tot = big.explore_sources(G, 0, K)
            t1 = time.perf_counter()
            if k:
                t_new.append(t1 - t0)
                sim.append(tot["sim_ms"])
                merge.append(tot["merge_ms"])
        assert tot["passes"] == 1 and tot["schedules"] == G * K
    one = np.zeros((K, 8, L), np.uint16), np.zeros((K, 8), np.uint32)
    per_source = []
    with dash.Engine(K, num_procs=8, cache_size=4, max_instr=L, schedule_seed=1, keep_state=True,
                     device=args.device) as old:
        for s in range(sample):
            one[0][0], one[1][0] = packed[s], lens[s]
            old.load_traces(*one)
            t0 = time.perf_counter()
            o = old.explore(0, 0, K)
            rec = old.check_outcomes(0, o)
            per_source.append(time.perf_counter() - t0)
            assert as_rows(outs, s) == old_rows(o, rec), s
    old_s = spread(per_source)
    out.update({"new_call_s": spread(t_new), "new_sim_ms": spread(sim), "new_merge_ms": spread(merge),
                "outcomes": tot["outcomes"], "table_slots": tot["table_slots"],
                "incoherent_schedule_share": tot["incoherent_schedules"] / tot["schedules"],
                "incoherent_clean_schedule_share": tot["incoherent_clean_schedules"] / tot["schedules"],
                "bit_names": list(dash.COH_NAMES), "bit_schedules": tot["bit_schedules"],
                "old_route_per_source_s": old_s, "old_route_sources_measured": sample,
                "old_route_scaled_to_all_sources_s": old_s["median"] * G,
                "old_route_is_scaled_not_measured": True, "lists_equal_for_the_measured_sources": True,
                "new_over_scaled_old": statistics.median(t_new) / (old_s["median"] * G)})
    print(json.dumps({"c": "many sources", "new_s": statistics.median(t_new), "old_scaled_s": old_s["median"] * G}),
          flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "explore_sources.json"))
    args = ap.parse_args()
    dash = load_package()
    out = {"tool": "tools/explore_sources_row.py", "reps": args.reps, "box": dash.probe_box(args.device)}
    path = pathlib.Path(args.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    for name, part in (("a", part_a), ("b", part_b), ("c", part_c)):
        if name in args.parts:
            out[{"a": "one_source", "b": "insert_kernel", "c": "many_sources"}[name]] = part(dash, args)
            path.write_text(json.dumps(out, indent=1) + "\n")  # what is measured so far
    print(json.dumps({"explore_sources_row": "ok", "out": args.out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
