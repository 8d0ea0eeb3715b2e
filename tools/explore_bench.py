#!/usr/bin/env python3
"""What a schedule seed per system costs, and how fast a trace directory's outcomes are explored.

Workload: the headline shape (--systems x 8 nodes x --len uniform instructions, CACHE_SIZE 4,
generated on the device). One process warms and then times, alternately, --reps runs each of
  (a) lockstep                      a handle created with schedule_seed = 0;
  (b) the handle-seeded schedule    schedule_seed = S, round words from the handle's table;
  (c) per-system seeds, all distinct (dash_set_system_seeds: round words hashed in the kernel);
kernel_ms is dash_stats.kernel_ms (device events around the run's launches). Reported: the
medians with their spread, (b) / (a) and (c) / (b).

--parent-pkg DIR (the package directory of a built checkout of the parent commit: its dash.py and
libdash.so) adds the regression check on (b): child processes, alternately on the parent's
package and on this tree's, --procs of each, time (b) the same way. The allowed difference is the
run-to-run spread of the parent itself (largest minus smallest of its processes' medians); both
figures and the verdict go into the JSON, and the digest checksums of the two builds must agree.

explore: wall time (host clock around dash_explore, which ends synchronised) of 2^20 seeds of
tests/golden/reference/test_4 at 4 nodes, on a 65,536-system handle (16 passes) and on a
2^20-system handle (one pass); the outcome list must be the same from both.
Writes profiles/explore.json (--out).

--micro times instead, in one alternating run, dash_explore_micro (seeded micro-step schedules,
uniform weights) and dash_explore (seeded round schedules) over the same 2^20 seeds of test_4 on
the same two handles, and the CPU checker's own weighted random walk (orc_random_walk, STRICT
model) on 16 host threads of the same box; schedules per second by the host clock and the outcome
counts go to profiles/explore_micro.json (--micro-out).
"""
import argparse
import importlib.util
import json
import os
import pathlib
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from __graft_entry__ import load_package  # noqa: E402

SCHED_SEED = 0x5EED5EED
GEN_SEED = 0x5EED


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def checksum(eng):
    d = eng.read_results()[0]
    return [int((d & np.uint64(0xFFFFFFFF)).sum(dtype=np.uint64)), int((d >> np.uint64(32)).sum(dtype=np.uint64))]


def seeded_only(dash, args):
    """(b) alone, for one library: the child process of the parent comparison."""
    with dash.Engine(args.systems, num_procs=8, cache_size=4, max_instr=args.len, device=args.device,
                     schedule_seed=SCHED_SEED) as eng:
        eng.generate(GEN_SEED, args.len, kind=dash.GEN_UNIFORM)
        eng.run()  # warm: code object, and the overflow hint of these traces
        eng.run()
        ks = [eng.run()["kernel_ms"] for _ in range(args.reps)]
        return {"kernel_ms": ks, "digest_sum": checksum(eng)}


def three_schedules(dash, args):
    n, L = args.systems, args.len
    seeds = (np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) | np.uint64(1)
    assert len(np.unique(seeds)) == n
    mk = lambda seed: dash.Engine(n, num_procs=8, cache_size=4, max_instr=L, device=args.device, schedule_seed=seed)
    with mk(0) as ea, mk(SCHED_SEED) as eb, mk(SCHED_SEED) as ec:
        engines = {"a_lockstep": ea, "b_handle_seed": eb, "c_per_system_seeds": ec}
        for eng in engines.values():
            eng.generate(GEN_SEED, L, kind=dash.GEN_UNIFORM)
        ec.set_system_seeds(seeds)
        for eng in engines.values():  # warm each kernel and each handle's overflow hint
            eng.run()
            eng.run()
        ms = {k: [] for k in engines}
        stats = {}
        for _ in range(args.reps):
            for k, eng in engines.items():
                stats[k] = eng.run()
                ms[k].append(stats[k]["kernel_ms"])
        # (c) with one seed everywhere must be (b): the hashing path against the table path
        ec.set_system_seeds(np.full(n, SCHED_SEED, dtype=np.uint64))
        ec.run()
        same = checksum(ec) == checksum(eb)
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"workload": f"{n} systems x 8 nodes x {L} uniform RD/WR per node, CACHE_SIZE 4, device generator",
            "kernel_ms": {k: spread(v) for k, v in ms.items()},
            "rounds_total": {k: stats[k]["rounds_total"] for k in stats},
            "wave_rounds": {k: stats[k]["wave_rounds"] for k in stats},
            "b_over_a": med["b_handle_seed"] / med["a_lockstep"],
            "c_over_b": med["c_per_system_seeds"] / med["b_handle_seed"],
            "one_seed_everywhere_equals_handle_seed": bool(same)}


def parent_check(args):
    pkgs = {"parent": args.parent_pkg, "this_tree": ROOT / "ue22cs343bb1-openmp-assignment_amd"}
    runs = {k: [] for k in pkgs}
    sums = {}
    env = dict(os.environ)
    env.pop("DASH_LIB", None)  # each package loads the library beside its dash.py
    for _ in range(args.procs):
        for k, pkg in pkgs.items():  # alternating
            p = subprocess.run([sys.executable, __file__, "--worker", str(pkg), "--systems", str(args.systems),
                                "--len", str(args.len), "--reps", str(args.reps), "--device", str(args.device)],
                               env=env, capture_output=True, text=True, check=True)
            r = json.loads(p.stdout.strip().splitlines()[-1])
            runs[k].append(r["kernel_ms"])
            sums.setdefault(k, r["digest_sum"])
    meds = {k: [statistics.median(x) for x in v] for k, v in runs.items()}
    parent_spread = max(meds["parent"]) - min(meds["parent"])
    diff = statistics.median(meds["this_tree"]) - statistics.median(meds["parent"])
    return {"what": "(b) on a build of the parent commit and on this tree, child processes alternating; "
                    "kernel_ms medians per process",
            "process_medians_ms": meds, "all_ms": runs,
            "parent_run_to_run_spread_ms": parent_spread, "this_tree_minus_parent_ms": diff,
            "not_slower_within_spread": diff <= parent_spread,
            "digest_sums_equal": sums["parent"] == sums["this_tree"]}


def explore_wall(dash, args):
    import oracle_ctypes as oc
    tr, lens = oc.load_test_dir(oc.GOLDEN / "test_4")
    total = 1 << 20
    out = {"what": f"dash_explore over {total} seeds of tests/golden/reference/test_4, 4 nodes; host clock, "
                   "the load of the handle not included"}
    lists = []
    for nsys in (1 << 16, 1 << 20):
        with dash.Engine(nsys, num_procs=4, cache_size=4, max_instr=32, device=args.device, schedule_seed=1) as eng:
            packed = np.zeros((nsys, 4, tr.shape[1]), np.uint16)
            ln = np.zeros((nsys, 4), np.uint32)
            packed[0], ln[0] = tr, lens
            eng.load_traces(packed, ln)
            eng.explore(0, 0, nsys)  # warm
            ts = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                got = eng.explore(0, 0, total)
                ts.append(time.perf_counter() - t0)
        lists.append(got)
        out[f"handle_{nsys}_systems"] = {"passes": total // nsys, "seconds": spread(ts),
                                         "schedules_per_s": total / statistics.median(ts)}
    out["outcomes"] = [dict(o, digest=f"{o['digest']:016x}") for o in lists[0]]
    out["same_list_from_both_handles"] = lists[0] == lists[1]
    return out


def oracle_walk_rate(tr, lens, threads=16, walks=32768):
    """orc_random_walk (uniform node weights, STRICT) on `threads` host threads: walks per second by
    the host clock, and the distinct outcomes seen. The library call releases the interpreter lock."""
    import concurrent.futures
    import ctypes
    import oracle_ctypes as oc
    L = oc.lib()
    tr, lens = oc._tr(tr, lens)

    def some(k):  # one thread's share, its buffers made once: the loop is the library call
        cfg = oc.OrcCfg(4, 4, 256, 0, 0, oc.MICRO_STRICT, 0)
        res, wit, wl = oc.OrcOutcome(), np.zeros(1 << 16, np.uint16), ctypes.c_uint32()
        digs = []
        for s in range(k, walks, threads):
            rc = L.orc_random_walk(ctypes.byref(cfg), tr.ctypes.data, tr.shape[1], lens.ctypes.data, 0, 1 + s, None,
                                   None, ctypes.addressof(res), wit.ctypes.data, len(wit), ctypes.addressof(wl))
            assert rc == 0
            digs.append(int(res.digest))
        return digs
    some(walks - 8)  # warm
    t0 = time.perf_counter()
    with concurrent.futures.ThreadPoolExecutor(threads) as ex:
        digs = [d for part in ex.map(some, range(threads)) for d in part]
    dt = time.perf_counter() - t0
    return {"threads": threads, "walks": len(digs), "seconds": dt, "walks_per_s": len(digs) / dt,
            "distinct_outcomes": len(set(digs)), "host_cpus": os.cpu_count()}


def explore_micro_wall(dash, args):
    import oracle_ctypes as oc
    tr, lens = oc.load_test_dir(oc.GOLDEN / "test_4")
    total = 1 << 20
    out = {"what": f"{total} schedules of tests/golden/reference/test_4 (4 nodes), seeds 1 .. 2^20: dash_explore_micro "
                   "(seeded micro-step schedules, uniform weights) and dash_explore (seeded round schedules) "
                   "alternating on each handle; host clock around the call, the load of the handle not included",
           "measured": "seconds, schedules_per_s, the outcome counts, rounds_of_last_pass (dash_stats), "
                       "oracle_random_walk",
           "counted_from_the_code": "passes = 2^20 / systems of the handle"}
    lists = {"micro": [], "rounds": []}
    for nsys in (1 << 16, 1 << 20):
        with dash.Engine(nsys, num_procs=4, cache_size=4, max_instr=32, device=args.device, schedule_seed=1) as eng:
            packed = np.zeros((nsys, 4, tr.shape[1]), np.uint16)
            ln = np.zeros((nsys, 4), np.uint32)
            packed[0], ln[0] = tr, lens
            eng.load_traces(packed, ln)
            kinds = {"micro": lambda k: eng.explore_micro(0, 1, k), "rounds": lambda k: eng.explore(0, 1, k)}
            for fn in kinds.values():
                fn(nsys)  # warm
            ts = {k: [] for k in kinds}
            got = {}
            for _ in range(args.reps):
                for k, fn in kinds.items():  # alternating
                    t0 = time.perf_counter()
                    got[k] = fn(total)
                    ts[k].append(time.perf_counter() - t0)
            rec = {"passes": total // nsys}
            for k in kinds:
                lists[k].append(got[k])
                rec[k] = {"seconds": spread(ts[k]), "schedules_per_s": total / statistics.median(ts[k]),
                          "distinct_outcomes": len(got[k])}
            eng.set_micro_seeds(np.arange(1, nsys + 1, dtype=np.uint64))
            st = eng.run()
            rec["micro_last_pass"] = {"kernel_ms": st["kernel_ms"], "rounds_total": st["rounds_total"],
                                      "rounds_max": st["rounds_max"], "err_bits": st["err_bits"]}
        out[f"handle_{nsys}_systems"] = rec
    for k, v in lists.items():
        out[f"{k}_outcomes"] = [dict(o, digest=f"{o['digest']:016x}") for o in v[0]]
        out[f"{k}_same_list_from_both_handles"] = v[0] == v[1]
    out["oracle_random_walk"] = oracle_walk_rate(tr, lens)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--systems", type=int, default=1 << 20)
    ap.add_argument("--len", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--procs", type=int, default=3, help="child processes per library of the parent comparison")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--parent-pkg", default=None)
    ap.add_argument("--worker", default=None, metavar="PKG", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "explore.json"))
    ap.add_argument("--micro", action="store_true", help="time dash_explore_micro against dash_explore instead")
    ap.add_argument("--micro-out", default=str(ROOT / "profiles" / "explore_micro.json"))
    args = ap.parse_args()
    if args.worker:  # (b) alone on the package in that directory
        spec = importlib.util.spec_from_file_location("dash_worker", pathlib.Path(args.worker) / "dash.py")
        dash = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(dash)
        print(json.dumps(seeded_only(dash, args)))
        return 0
    dash = load_package()
    assert args.reps >= 5, "at least five timings of each schedule"
    out = {"tool": "tools/explore_bench.py", "reps": args.reps,
           "box": {k: v for k, v in dash.probe_box(args.device).items() if k in ("name", "arch", "compute_units")}}
    if args.micro:
        out["explore_micro"] = explore_micro_wall(dash, args)
        ok = out["explore_micro"]["micro_same_list_from_both_handles"] and \
            out["explore_micro"]["rounds_same_list_from_both_handles"]
        pathlib.Path(args.micro_out).write_text(json.dumps(out, indent=1) + "\n")
        print(json.dumps({"explore_bench": "ok" if ok else "RESULTS DIFFER", "out": args.micro_out}))
        return 0 if ok else 1
    out["schedules"] = three_schedules(dash, args)
    print(json.dumps({k: out["schedules"][k] for k in ("b_over_a", "c_over_b")}), flush=True)
    out["explore"] = explore_wall(dash, args)
    print(json.dumps({"explore": out["explore"]["handle_65536_systems"]["seconds"]}), flush=True)
    ok = out["schedules"]["one_seed_everywhere_equals_handle_seed"] and out["explore"]["same_list_from_both_handles"]
    if args.parent_pkg:
        out["parent_comparison"] = parent_check(args)
        ok = ok and out["parent_comparison"]["digest_sums_equal"]
        print(json.dumps({k: out["parent_comparison"][k] for k in
                          ("parent_run_to_run_spread_ms", "this_tree_minus_parent_ms", "not_slower_within_spread")}),
              flush=True)
    else:
        out["parent_comparison"] = "not measured (no --parent-pkg given)"
    pathlib.Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({"explore_bench": "ok" if ok else "RESULTS DIFFER", "out": args.out}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
