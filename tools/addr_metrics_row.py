#!/usr/bin/env python3
"""What dash_compute_addr_metrics costs, against dash_compute_metrics over the same log and against
the route a user had before it existed.

Workload, per --kinds entry (uniform, contention): --systems x 8 nodes x --len instructions,
CACHE_SIZE 4, generated on the device, run with an event log that holds every round. A first handle
without a log finds the longest run; the timed handle's log is sized to it. If that log does not fit
the device, the systems are halved until it does, and the figure used is written down.

(a) kernels: dash_compute_addr_metrics and dash_compute_metrics, each between two device events on the
    handle's stream (the events enclose the totals' memset, the kernel and the copy of the totals),
    in the same process on the same log, in alternating order (address first on even repeats, node
    first on odd ones), after --warmup rounds, --reps times each. Bytes of log read = sum over systems
    of ceil4(K) * num_procs * 4, K = min(rounds, the log's rounds); rate = bytes / median time, as a
    fraction of the HBM peak (8 TB/s).
(b) the old route: for the first --sample systems, dash_read_events (the device-to-host copy of one
    system's log and its merge into an event list) and dash_addr_metrics_from_events (the host's pass),
    each on the host clock, through ctypes without any Python per event. The batch figure is a scaling,
    written out as one: seconds per sampled system x systems, one host thread.
Every figure goes to --out (profiles/addr_metrics.json) with the box probe."""
import argparse
import ctypes
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


def timed(stream, torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    out = fn()  # returns with the stream synchronised
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), out


def old_route(dash, eng, sample, N, rounds):
    """dash_read_events + dash_addr_metrics_from_events for systems [0, sample): seconds of each, and the
    records for a comparison with the kernel's."""
    L = dash.lib()
    read_s, pass_s, recs = [], [], []
    for s in range(sample):
        n = ctypes.c_uint32()
        t0 = time.perf_counter()
        rc = L.dash_read_events(eng.h, s, None, 0, ctypes.byref(n))
        assert rc == dash.OK, rc
        arr = (dash.Event * max(n.value, 1))()
        rc = L.dash_read_events(eng.h, s, arr, n.value, ctypes.byref(n))
        assert rc == dash.OK, rc
        t1 = time.perf_counter()
        rec = np.zeros(N * 16, dtype=dash.ADDR_METRICS_DTYPE)
        rc = L.dash_addr_metrics_from_events(arr, n.value, N, int(rounds[s]), rec.ctypes.data, None)
        assert rc == dash.OK, rc
        t2 = time.perf_counter()
        read_s.append(t1 - t0)
        pass_s.append(t2 - t1)
        recs.append(rec)
    return read_s, pass_s, np.stack(recs)


def measure(dash, torch, kind_name, kind, n, L, args):
    N, CS = 8, 4
    with dash.Engine(n, num_procs=N, cache_size=CS, max_instr=L, device=args.device) as eng:
        eng.generate(GEN_SEED, L, kind=kind)
        longest = eng.run()["rounds_max"]
    with dash.Engine(n, num_procs=N, cache_size=CS, max_instr=L, device=args.device, trace_events=longest) as eng:
        eng.generate(GEN_SEED, L, kind=kind)
        stats = eng.run()
        rounds = eng.read_results()[1].astype(np.int64)
        ev_rounds = (longest + 3) & ~3
        log_bytes = int(((np.minimum(rounds, ev_rounds) + 3) // 4 * 4).sum()) * N * 4
        stream = torch.cuda.ExternalStream(eng.stream(), device=args.device)
        ms = {"addr": [], "node": []}
        calls = {"addr": eng.compute_addr_metrics, "node": eng.compute_metrics}
        for k in range(args.warmup + args.reps):
            for which in (("addr", "node") if k % 2 == 0 else ("node", "addr")):
                t, tot = timed(stream, torch, calls[which])
                if k >= args.warmup:
                    ms[which].append(t)
                if which == "addr":
                    addr_tot = tot
                else:
                    node_tot = tot
        assert addr_tot["systems"] == n and addr_tot["truncated_systems"] == 0 and addr_tot["foreign_events"] == 0
        assert addr_tot["reads"] + addr_tot["writes"] == stats["instructions"] and addr_tot["msgs"] == sum(stats["hist"])
        for f in ("reads", "writes", "read_misses", "write_misses", "upgrades", "invalidations", "interventions",
                  "evict_shared", "evict_modified", "msgs"):
            assert addr_tot[f] == node_tot[f], f
        sample = min(args.sample, n)
        read_s, pass_s, host_rec = old_route(dash, eng, sample, N, rounds)
        assert np.array_equal(host_rec, eng.read_addr_metrics(0, sample)[0])
    a_ms, m_ms = statistics.median(ms["addr"]), statistics.median(ms["node"])
    per_sys = statistics.mean(read_s) + statistics.mean(pass_s)
    row = {"workload": f"{n} systems x {N} nodes x {L} {kind_name} RD/WR per node, CACHE_SIZE {CS}, device generator, "
                       f"event log of {longest} rounds",
           "systems": n, "log_bytes_read": log_bytes, "kernel_ms_of_the_logged_run": stats["kernel_ms"],
           "addr_kernel": {"what": "dash_compute_addr_metrics between device events on the handle's stream",
                           "ms": spread(ms["addr"]), "bytes_per_s": log_bytes / (a_ms * 1e-3),
                           "fraction_of_hbm_peak": log_bytes / (a_ms * 1e-3) / HBM_PEAK, "totals": addr_tot},
           "node_kernel": {"what": "dash_compute_metrics on the same log, same process, alternating order",
                           "ms": spread(ms["node"]), "bytes_per_s": log_bytes / (m_ms * 1e-3),
                           "fraction_of_hbm_peak": log_bytes / (m_ms * 1e-3) / HBM_PEAK},
           "addr_over_node": a_ms / m_ms,
           "addr_minus_node_ms": a_ms - m_ms,
           "spread_of_the_runs_ms": max(max(ms["addr"]) - min(ms["addr"]), max(ms["node"]) - min(ms["node"])),
           "old_route": {"what": "dash_read_events + dash_addr_metrics_from_events per system, host clock, one thread, "
                                 "ctypes arrays (no Python per event); records equal the kernel's",
                         "sampled_systems": sample, "read_events_s_per_system": spread(read_s),
                         "host_pass_s_per_system": spread(pass_s),
                         "scaled_to_the_batch_s": per_sys * n,
                         "scaling": f"(mean read_events s + mean host pass s) x {n} systems = {per_sys:.6f} x {n}",
                         "over_the_kernel": per_sys * n / (a_ms * 1e-3)}}
    print(json.dumps({"kind": kind_name, "systems": n, "addr_ms": a_ms, "node_ms": m_ms,
                      "addr_fraction_of_hbm_peak": row["addr_kernel"]["fraction_of_hbm_peak"],
                      "old_route_scaled_s": per_sys * n}), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--systems", type=int, default=32768)
    ap.add_argument("--len", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sample", type=int, default=16, help="systems the old route is timed on")
    ap.add_argument("--kinds", default="uniform,contention")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "addr_metrics.json"))
    args = ap.parse_args()
    assert args.reps >= 5, "the median of at least five runs"
    import torch
    dash = load_package()
    torch.cuda.set_device(args.device)
    kinds = {"uniform": dash.GEN_UNIFORM, "contention": dash.GEN_CONTENTION}
    out = {"tool": "tools/addr_metrics_row.py", "box": dash.probe_box(args.device), "reps": args.reps,
           "warmup": args.warmup, "hbm_peak_bytes_per_s": HBM_PEAK, "rows": {}}
    for name in args.kinds.split(","):
        n = args.systems
        while True:
            try:
                out["rows"][name] = measure(dash, torch, name, kinds[name], n, args.len, args)
                break
            except dash.DashError as e:  # the log of this many systems does not fit: halve them
                if e.code != dash.ENOMEM or n <= 1024:
                    raise
                n //= 2
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({"addr_metrics_row": "ok", "out": args.out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
