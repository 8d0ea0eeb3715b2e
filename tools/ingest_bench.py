#!/usr/bin/env python3
"""Host-parsed against device-parsed trace-directory ingest, on the project's ingest workload
(bench_next.py: 2,048 directories x 8 core_<n>.txt x 4,096 lines), and the same at 4 nodes.

Both paths are warmed, then timed alternately in one process (host clock around the
synchronising call, --reps times each). Reported, each named for what it is:
  end_to_end   lines/s and text MB/s of load_dirs and of load_dirs(device=True), with the spread,
               and their ratio (device over host, from the medians);
  stages       dash_ingest_info of the device path: host file reads (wall clock of the reader
               phases), H2D copies and the parse kernel (device events); reads overlap the other two;
  kernel       the parse kernel alone (device events around its one launch in load_text):
               text bytes/s, and (text bytes read + packed bytes written) per second as a share
               of the HBM peak. A kernel figure, not an ingest rate;
  load_text    Engine.load_text from an in-memory slab (no file reads), end to end;
  parity       digests, rounds and errors of a run after each path, equal for every system.
Writes profiles/ingest_device.json (--out).
"""
import argparse
import json
import pathlib
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import bench_next  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402

HBM_PEAK_BYTES_PER_S = 8.0e12  # MI355X HBM3E, datasheet peak


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def one_shape(dash, dev, seed, systems, N, L, reps, workdir):
    rng = np.random.default_rng(seed)
    packed = rng.bit_generator.random_raw(systems * N * L // 4).view(np.uint16).reshape(systems, N, L).copy()
    if N < 8:  # keep every address homed on a node < N (bits 14..12 of a word name the node)
        node = ((packed >> 12) & 7) % N
        packed = (packed & 0x8FFF) | (node << 12).astype(np.uint16)
    dirs = bench_next.write_dirs(workdir, packed)
    blobs = [[(d / f"core_{t}.txt").read_bytes() for t in range(N)] for d in dirs]
    text_bytes = sum(len(b) for row in blobs for b in row)
    lines = systems * N * L
    t_host, t_dev, t_text, stages, kernel_ms = [], [], [], [], []
    with dash.Engine(systems, num_procs=N, cache_size=4, max_instr=L, device=dev) as eng:
        eng.load_dirs(dirs)               # warm: page cache, host threads, device buffers
        eng.load_dirs(dirs, device=True)  # warm: pinned slabs, the kernel's code object
        for _ in range(reps):
            t0 = time.perf_counter()
            eng.load_dirs(dirs)
            t_host.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            eng.load_dirs(dirs, device=True)
            t_dev.append(time.perf_counter() - t0)
            stages.append(eng.ingest_info())
        eng.load_dirs(dirs)
        eng.run()
        res_host = eng.read_results()
        eng.load_dirs(dirs, device=True)
        eng.run()
        res_dev = eng.read_results()
        slab, off, ln = dash.pack_text([b for row in blobs for b in row])
        eng.load_text_slab(slab, off, ln)  # warm
        for _ in range(reps):
            t0 = time.perf_counter()
            eng.load_text_slab(slab, off, ln)
            t_text.append(time.perf_counter() - t0)
            kernel_ms.append(eng.ingest_info()["parse_ms"])
        eng.run()
        res_text = eng.read_results()
    parity = all(np.array_equal(a, b) and np.array_equal(a, c) for a, b, c in zip(res_host, res_dev, res_text))
    rate = lambda ts: {"seconds": spread(ts), "lines_per_s": lines / statistics.median(ts),
                       "text_MB_per_s": text_bytes / statistics.median(ts) / 1e6}
    k_s = statistics.median(kernel_ms) / 1e3
    moved = text_bytes + lines * 2
    return {
        "workload": f"{systems} trace directories x {N} core_<n>.txt x {L} lines ({text_bytes / 1e6:.0f} MB of text)",
        "end_to_end": {"host_load_dirs": rate(t_host), "device_load_dirs": rate(t_dev),
                       "device_over_host": statistics.median(t_host) / statistics.median(t_dev),
                       "device_not_slower": statistics.median(t_dev) <= statistics.median(t_host)},
        "stages_device_path_ms": {k: spread([s[k] for s in stages]) for k in ("read_ms", "copy_ms", "parse_ms")},
        "kernel": {"what": "the parse kernel alone, device events around its single launch in load_text; "
                           "a kernel figure, not an ingest rate",
                   "ms": spread(kernel_ms), "text_bytes_per_s": text_bytes / k_s,
                   "bytes_moved_per_s": moved / k_s, "share_of_hbm_peak": moved / k_s / HBM_PEAK_BYTES_PER_S,
                   "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S},
        "load_text_in_memory": rate(t_text),
        "parity_digests_rounds_errors_equal": bool(parity),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--systems", type=int, default=2048)
    ap.add_argument("--len", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--seed", type=int, default=0x5EED)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ingest_device.json"))
    args = ap.parse_args()
    assert args.reps >= 5, "at least five timings of each path"
    dash = load_package()
    out = {"tool": "tools/ingest_bench.py", "reps": args.reps,
           "box": {k: v for k, v in dash.probe_box(args.device).items() if k in ("name", "arch", "compute_units")}}
    for N in (8, 4):
        with tempfile.TemporaryDirectory() as td:
            out[f"nodes_{N}"] = one_shape(dash, args.device, args.seed, args.systems, N, args.len, args.reps, td)
        print(json.dumps({f"nodes_{N}": out[f"nodes_{N}"]["end_to_end"]}), flush=True)
    pathlib.Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    ok = all(out[f"nodes_{N}"]["parity_digests_rounds_errors_equal"] for N in (8, 4))
    print(json.dumps({"ingest_bench": "ok" if ok else "PARITY FAILED", "out": args.out}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
