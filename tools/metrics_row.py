#!/usr/bin/env python3
"""What dash_compute_metrics costs, against the route a user had before it existed.

Workload: --systems x 8 nodes x --len uniform instructions, CACHE_SIZE 4, generated on the device,
run with an event log that holds every round (the README's DEBUG-log row). A first handle without a
log finds the longest run; the timed handle's log is sized to it.

(a) kernel: dash_compute_metrics between two device events on the handle's stream (the events
    enclose the totals' memset, the kernel and the 144-B copy of the totals), after --warmup calls,
    --reps times. Bytes of log read = sum over systems of ceil4(K) * num_procs * 4, K = min(rounds,
    the log's rounds); rate = bytes / median time, as a fraction of the HBM peak (8 TB/s).
(b) the old route, in this tool and not in the library: one device-to-host copy of as many bytes
    into pinned host memory, timed by device events, and a 16-thread host pass over them (numpy,
    which releases the interpreter lock) that only counts events by kind and message type -- less
    than the per-node records the kernel leaves, so the comparison favours the old route. The
    library does not give out the log's device address, so the copy's source is a device buffer of
    this tool's own with the same size and layout, filled with the log rows of the first --sample
    systems (rebuilt from dash_read_events) repeated.
The kernel reads from HBM what (b) moves over the host link, so it has to beat (b)'s copy alone;
the verdict and every figure go to --out (profiles/metrics.json) with the box probe."""
import argparse
import concurrent.futures
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
EV_EVENT, EV_INSTR = 1 << 24, 1 << 31


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def rows_of(eng, s, rounds, N):
    """System s's log rows [round / 4][node][round % 4] as the device holds them (the bits
    dash_read_events drops left out), for ceil4(rounds) rounds."""
    rows = np.zeros(((rounds + 3) // 4, N, 4), np.uint32)
    for e in eng.read_events(s):
        rows[e.round // 4, e.node, e.round % 4] = e.word | EV_EVENT | (EV_INSTR if e.kind else 0)
    return rows.reshape(-1)


def host_pass(words, threads=16):
    """Counts over the copied words on `threads` host threads: instructions, and messages by type."""
    def part(k):
        lo, hi = len(words) * k // threads, len(words) * (k + 1) // threads
        instr, hist = 0, np.zeros(16, np.int64)
        for a in range(lo, hi, 1 << 22):
            w = words[a:min(hi, a + (1 << 22))]
            ev = (w & EV_EVENT) != 0
            ins = ev & ((w & EV_INSTR) != 0)
            instr += int(ins.sum())
            hist += np.bincount(w[ev & ~ins] & 15, minlength=16)
        return instr, hist
    with concurrent.futures.ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(part, range(threads)))
    return sum(p[0] for p in parts), sum(p[1] for p in parts)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--systems", type=int, default=32768)
    ap.add_argument("--len", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sample", type=int, default=16, help="systems whose real rows fill the old route's buffer")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "metrics.json"))
    args = ap.parse_args()
    assert args.reps >= 5, "the median of at least five runs"
    import torch
    dash = load_package()
    N, CS, n, L = 8, 4, args.systems, args.len
    torch.cuda.set_device(args.device)
    box = dash.probe_box(args.device)
    with dash.Engine(n, num_procs=N, cache_size=CS, max_instr=L, device=args.device) as eng:
        eng.generate(GEN_SEED, L, kind=dash.GEN_UNIFORM)
        longest = eng.run()["rounds_max"]
    out = {"tool": "tools/metrics_row.py",
           "workload": f"{n} systems x {N} nodes x {L} uniform RD/WR per node, CACHE_SIZE {CS}, device generator, "
                       f"event log of {longest} rounds",
           "box": box, "reps": args.reps, "warmup": args.warmup}
    with dash.Engine(n, num_procs=N, cache_size=CS, max_instr=L, device=args.device, trace_events=longest) as eng:
        eng.generate(GEN_SEED, L, kind=dash.GEN_UNIFORM)
        eng.run()
        stats = eng.run()
        rounds = eng.read_results()[1].astype(np.int64)
        ev_rounds = (longest + 3) & ~3
        log_bytes = int(((np.minimum(rounds, ev_rounds) + 3) // 4 * 4).sum()) * N * 4
        stream = torch.cuda.ExternalStream(eng.stream(), device=args.device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for k in range(args.warmup + args.reps):
            e0.record(stream)
            tot = eng.compute_metrics()  # returns with the stream synchronised
            e1.record(stream)
            e1.synchronize()
            if k >= args.warmup:
                ms.append(e0.elapsed_time(e1))
        assert tot["systems"] == n and tot["truncated_systems"] == 0
        assert tot["reads"] + tot["writes"] == stats["instructions"] and tot["msgs"] == sum(stats["hist"])
        k_ms = statistics.median(ms)
        out["kernel"] = {"what": "dash_compute_metrics between device events on the handle's stream",
                         "ms": spread(ms), "log_bytes_read": log_bytes, "bytes_per_s": log_bytes / (k_ms * 1e-3),
                         "fraction_of_hbm_peak": log_bytes / (k_ms * 1e-3) / HBM_PEAK, "hbm_peak_bytes_per_s": HBM_PEAK,
                         "kernel_ms_of_the_logged_run": stats["kernel_ms"], "totals": tot}
        print(json.dumps({"kernel_ms": k_ms, "fraction_of_hbm_peak": out["kernel"]["fraction_of_hbm_peak"]}), flush=True)
        sample = np.concatenate([rows_of(eng, s, int(rounds[s]), N) for s in range(min(args.sample, n))])
    # (b) the old route: the same number of bytes to pinned host memory, then 16 host threads
    words = log_bytes // 4
    host_src = np.resize(sample, words)
    dev = torch.from_numpy(host_src.view(np.int32)).to(f"cuda:{args.device}")
    pinned = torch.empty(words, dtype=torch.int32).pin_memory()
    c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    copy_ms = []
    for k in range(args.warmup + args.reps):
        c0.record()
        pinned.copy_(dev, non_blocking=True)
        c1.record()
        c1.synchronize()
        if k >= args.warmup:
            copy_ms.append(c0.elapsed_time(c1))
    view = pinned.numpy().view(np.uint32)
    assert np.array_equal(view[:len(sample)], sample[:words])
    red_s = []
    for _ in range(3):
        t0 = time.perf_counter()
        instr, hist = host_pass(view)
        red_s.append(time.perf_counter() - t0)
    c_ms = statistics.median(copy_ms)
    out["old_route"] = {"what": "device-to-host copy of log_bytes_read bytes into pinned memory (device events), then "
                                "a 16-thread numpy pass counting instructions and messages by type (host clock)",
                        "source_buffer": f"rows of the first {min(args.sample, n)} systems, repeated",
                        "copy_ms": spread(copy_ms), "copy_bytes_per_s": log_bytes / (c_ms * 1e-3),
                        "host_pass_s": spread(red_s), "host_threads": 16,
                        "host_pass_counts": {"instructions": int(instr), "messages": int(hist.sum())}}
    out["kernel_over_copy_alone"] = k_ms / c_ms
    out["kernel_beats_the_copy_alone"] = bool(k_ms < c_ms)
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({"metrics_row": "ok" if out["kernel_beats_the_copy_alone"] else "KERNEL SLOWER THAN THE COPY",
                      "kernel_ms": k_ms, "copy_ms": c_ms, "host_pass_s": statistics.median(red_s), "out": args.out}))
    return 0 if out["kernel_beats_the_copy_alone"] else 1


if __name__ == "__main__":
    sys.exit(main())
