#!/usr/bin/env python3
"""What dash_shrink costs, against the route a user had before it existed, in one process.

Input: --systems generated systems x 8 nodes x --len uniform instructions (CACHE_SIZE 4, generated on the
device, lockstep); the first of them that ends incoherent with no error bit is shrunk under the goal "the
lowest bit of its record, no error bit", on the same handle of --systems systems.

(a) dash_shrink: a host clock around the call (it returns with the stream synchronised), and its report:
    sim_ms / gen_ms / select_ms (device events), rounds, variants, dash_run calls. Bytes the candidate
    kernel writes are computed here from the steps: per sub-pass systems x nodes x written chunks x 8 B
    (csrc/dash_shrink.hip, base_wchunks: the chunks of the base's longest trace plus two); gen_ms also holds
    the apply launches and the two copies of the base, so bytes / gen_ms understates the kernel's own rate.
    The call is the one-job case of the engine that dash_shrink_many runs.
(b) the old route, in this tool: per round the host builds every candidate of the base into a whole-batch
    buffer (numpy; stride = the base's longest trace), then dash_load_traces, dash_run,
    dash_check_coherence, dash_read_coherence and dash_read_results per sub-pass, selection in numpy.
Both start from the same traces (the old route's from the generator on a handle of one system) and must
give identical steps and final traces. --reps alternating rounds of (a) and (b), fewer when --budget-s runs
out (reps_done says how many); medians. Nothing is gated: the figures go to --out
(profiles/shrink.json) with the box probe. If the input needs more than --max-rounds rounds the tool says
so and stops: measure at a shorter --len, the rule stays as it is."""
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

HBM_PEAK = 8.0e12  # bytes/s, MI355X
GEN_SEED = 0x5EED


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def candidates(lens):
    """include/dash.h's enumeration: [(node, start, count)] in index order."""
    out = []
    for t, L in enumerate(int(x) for x in lens):
        if L:
            for j in range((L - 1).bit_length(), -1, -1):
                out += [(t, s, min(1 << j, L - s)) for s in range(0, L, 1 << j)]
    return out


def nchunks_of(max_instr):
    """dash_create's lane stride in 8-B chunks: an odd number of 128-B lines."""
    lines = (((max_instr + 3) // 4) * 8 + 127) // 128
    return (lines + (1 if lines and lines % 2 == 0 else 0)) * 16


def written_bytes(lens0, steps, S, N, max_instr):
    """Bytes the variant kernel stores into the trace buffer over a call: the copy for the check of the
    source, every sub-pass, the final copy."""
    nch, ln, total = nchunks_of(max_instr), [int(x) for x in lens0], 0
    w = lambda: max(1, min(nch, (max(ln) + 3) // 4 + 2))
    total += S * N * w() * 8
    for t, _s, n, C in steps:
        total += -(-int(C) // S) * S * N * w() * 8
        ln[int(t)] -= int(n)
    total += -(-len(candidates(ln)) // S) * S * N * w() * 8  # the last round, in which nothing passed
    total += S * N * w() * 8
    return total


def old_route(dash, eng, tr0, ln0, bit):
    """The shrink loop with every round's variants built on the host. Returns (trace, lens, steps, times)."""
    S, N = eng.num_systems, eng.num_procs
    tr, ln, steps = tr0.copy(), ln0.copy(), []
    t_build = t_load = t_run = t_read = 0.0
    while True:
        cands = candidates(ln)
        if not cands:
            break
        stride = max(int(ln.max()), 1)
        best = 0
        for first in range(0, len(cands), S):
            part = cands[first:first + S]
            t0 = time.perf_counter()
            buf = np.empty((S, N, stride), np.uint16)
            buf[:] = tr[None, :, :stride]
            lens = np.empty((S, N), np.uint32)
            lens[:] = ln
            for k, (t, s, n) in enumerate(part):
                L = int(ln[t])
                buf[k, t, s:L - n] = tr[t, s + n:L]
                buf[k, t, L - n:L] = 0
                lens[k, t] = L - n
            t1 = time.perf_counter()
            eng.load_traces(buf, lens)
            t2 = time.perf_counter()
            eng.run()
            eng.check_coherence()
            t3 = time.perf_counter()
            rec = eng.read_coherence(0, len(part))
            err = eng.read_results(0, len(part))[2]
            ok = ((rec["bits"] & bit) == bit) & (err == 0)
            count = np.array([n for _, _, n in part], np.uint64)
            key = np.where(ok, count << np.uint64(32) | (np.uint64(0xFFFFFFFF) - np.arange(first, first + len(part), dtype=np.uint64)),
                           np.uint64(0))
            best = max(best, int(key.max()))
            t4 = time.perf_counter()
            t_build += t1 - t0
            t_load += t2 - t1
            t_run += t3 - t2
            t_read += t4 - t3
        if best == 0:
            break
        t, s, n = cands[0xFFFFFFFF - (best & 0xFFFFFFFF)]
        steps.append((t, s, n, len(cands)))
        L = int(ln[t])
        tr[t, s:L - n] = tr[t, s + n:L].copy()
        tr[t, L - n:L] = 0
        ln[t] = L - n
    return tr, ln, steps, {"host_build_s": t_build, "load_traces_s": t_load, "run_and_check_s": t_run,
                           "read_and_select_s": t_read}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--systems", type=int, default=65536)
    ap.add_argument("--len", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-rounds", type=int, default=400)
    ap.add_argument("--budget-s", type=float, default=0, help="start no further alternating round after this many "
                                                             "seconds of them (0: all --reps)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "shrink.json"))
    args = ap.parse_args()
    dash = load_package()
    N, CS, S, L = 8, 4, args.systems, args.len
    box = dash.probe_box(args.device)
    out = {"tool": "tools/shrink_row.py",
           "workload": f"one of {S} generated systems x {N} nodes x {L} uniform RD/WR per node, CACHE_SIZE {CS}, "
                       f"lockstep, shrunk on a handle of {S} systems (DASH_KEEP_STATE)",
           "systems": S, "len": L, "box": box, "reps_asked": args.reps}
    with dash.Engine(S, num_procs=N, cache_size=CS, max_instr=L, device=args.device, keep_state=True) as eng:
        eng.generate(GEN_SEED, L, kind=dash.GEN_UNIFORM)
        eng.run()
        eng.check_coherence()
        rec, err = eng.read_coherence(), eng.read_results()[2]
        src = int(np.flatnonzero((rec["bits"] != 0) & (err == 0))[0])
        bit = int(rec["bits"][src]) & -int(rec["bits"][src])
        # the source's words for the old route: the generator again, on a handle of one system
        with dash.Engine(1, num_procs=N, cache_size=CS, max_instr=L, device=args.device) as one:
            one.generate(GEN_SEED, L, kind=dash.GEN_UNIFORM, sys_base=src)
            one_tr, one_ln = one.read_traces()
        tr0, ln0 = one_tr[0].copy(), one_ln[0].copy()
        out["input"] = {"system": src, "record_bits": int(rec["bits"][src]), "goal_bit": bit, "instr": int(ln0.sum()),
                        "candidates_of_the_first_round": len(candidates(ln0))}
        # one untimed call of (a): code objects loaded, buffers allocated; it also says how many rounds there are
        first = eng.shrink(src, bit, cap=args.max_rounds)
        if first["report"]["rounds"] > args.max_rounds:
            print(json.dumps({"shrink_row": "TOO MANY ROUNDS", "rounds": first["report"]["rounds"], "len": L}))
            return 1
        steps_a = [tuple(int(x) for x in s) for s in first["steps"]]
        new_s, old_s, reports, old_parts = [], [], [], []
        t_start = time.perf_counter()
        for _ in range(args.reps):
            if new_s and args.budget_s and time.perf_counter() - t_start > args.budget_s:
                break
            eng.generate(GEN_SEED, L, kind=dash.GEN_UNIFORM)  # the source back in place (untimed)
            t0 = time.perf_counter()
            got = eng.shrink(src, bit, cap=args.max_rounds)
            new_s.append(time.perf_counter() - t0)
            reports.append(got["report"])
            assert [tuple(int(x) for x in s) for s in got["steps"]] == steps_a
            t0 = time.perf_counter()
            tr_b, ln_b, steps_b, parts = old_route(dash, eng, tr0, ln0, bit)
            old_s.append(time.perf_counter() - t0)
            old_parts.append(parts)
            assert steps_b == steps_a and ln_b.tolist() == got["lens"].tolist(), "the two routes disagree"
            assert np.array_equal(tr_b, got["trace"][:, :tr_b.shape[1]])
            print(json.dumps({"dash_shrink_s": new_s[-1], "old_route_s": old_s[-1], "rounds": len(steps_a)}), flush=True)
    rep = reports[0]
    med = lambda f: spread([r[f] for r in reports])
    bytes_written = written_bytes(ln0, steps_a, S, N, L)
    gen_ms = med("gen_ms")["median"]
    out["dash_shrink"] = {"what": "host clock around dash_shrink (returns synchronised); report fields by device events",
                          "total_s": spread(new_s), "sim_ms": med("sim_ms"), "gen_ms": med("gen_ms"),
                          "select_ms": med("select_ms"), "rounds": rep["rounds"], "variants": rep["variants"],
                          "dash_run_calls": rep["passes"], "instr_before": rep["instr_before"],
                          "instr_after": rep["instr_after"], "host_bytes_read_per_round": 8,
                          "variant_kernel_bytes_written": bytes_written,
                          "variant_bytes_per_s_over_gen_ms": bytes_written / (gen_ms * 1e-3),
                          "fraction_of_hbm_peak": bytes_written / (gen_ms * 1e-3) / HBM_PEAK, "hbm_peak_bytes_per_s": HBM_PEAK}
    out["old_route"] = {"what": "per round: numpy builds every candidate into a whole-batch buffer, dash_load_traces, "
                                "dash_run, dash_check_coherence, dash_read_coherence, dash_read_results, numpy selection "
                                "(host clock)",
                        "total_s": spread(old_s),
                        **{k: spread([p[k] for p in old_parts]) for k in old_parts[0]}}
    out["reps_done"] = len(new_s)
    out["steps_identical_in_every_round"] = True
    out["old_over_new"] = statistics.median(old_s) / statistics.median(new_s)
    out["steps"] = [list(s) for s in steps_a]
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({"shrink_row": "ok", "dash_shrink_s": statistics.median(new_s), "old_route_s": statistics.median(old_s),
                      "old_over_new": out["old_over_new"], "rounds": rep["rounds"], "variants": rep["variants"],
                      "instr": [rep["instr_before"], rep["instr_after"]], "out": args.out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
