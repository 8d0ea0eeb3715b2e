#!/usr/bin/env python3
"""What dash_check_coherence costs, against the route a user had before it existed.

Workload: --systems x 8 nodes x --len uniform instructions, CACHE_SIZE 4, generated on the device,
run under lockstep on a handle with DASH_KEEP_STATE (2^20 systems: about 671 MB of final state).

(a) kernel: dash_check_coherence between two device events on the handle's stream (the events
    enclose the totals' memset, the kernel and the 160-B copy of the totals), after --warmup calls,
    --reps times. Bytes of state read = systems * num_procs * (16 + CACHE_SIZE) * 4; rate = bytes /
    median time, as a fraction of the HBM peak (8 TB/s). Reported, not gated.
(b) the old route, in this tool and not in the library: one device-to-host copy of as many bytes
    into pinned host memory, timed by device events, then a 16-thread host pass that unpacks the
    state words into dash_node_state records (numpy) and calls dash_check_states once per system.
    The library does not give out the state's device address, so the copy's source is a device
    buffer of this tool's own with the same size and layout, filled with the state words of the
    first --sample systems (rebuilt from dash_read_state) repeated; the host pass's records of those
    systems must equal the kernel's.
The kernel reads from HBM what (b) moves over the host link, so it has to beat (b)'s copy alone: the
only gate. The verdict, every figure and the workload's share of violating systems without an error
bit go to --out (profiles/coherence.json) with the box probe."""
import argparse
import concurrent.futures
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
NODE_DTYPE = np.dtype([("memory", np.uint8, 16), ("dir_bitvector", np.uint8, 16), ("dir_state", np.uint8, 16),
                       ("cache_addr", np.uint8, 16), ("cache_value", np.uint8, 16), ("cache_state", np.uint8, 16)])


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def words_of(nodes, CS):
    """One system's state words as the device holds them: per node 16 directory words (memory,
    bitvector << 8, state << 16), then CACHE_SIZE line words (address, value << 8, state << 16)."""
    out = []
    for s in nodes:
        out += [s.memory[b] | s.dir_bitvector[b] << 8 | s.dir_state[b] << 16 for b in range(16)]
        out += [s.cache_addr[i] | s.cache_value[i] << 8 | s.cache_state[i] << 16 for i in range(CS)]
    return np.array(out, np.uint32)


def unpack(words, N, CS):
    """State words [systems * N * (16 + CS)] as dash_node_state records [systems, N]."""
    w = words.reshape(-1, N, 16 + CS)
    nodes = np.zeros(w.shape[:2], NODE_DTYPE)
    nodes["cache_addr"][:] = 0xFF
    nodes["cache_state"][:] = 3
    nodes["memory"] = w[:, :, :16] & 0xFF
    nodes["dir_bitvector"] = (w[:, :, :16] >> 8) & 0xFF
    nodes["dir_state"] = (w[:, :, :16] >> 16) & 3
    nodes["cache_addr"][:, :, :CS] = w[:, :, 16:] & 0xFF
    nodes["cache_value"][:, :, :CS] = (w[:, :, 16:] >> 8) & 0xFF
    nodes["cache_state"][:, :, :CS] = (w[:, :, 16:] >> 16) & 3
    return nodes


def host_pass(dash, words, nsys, N, CS, threads=16):
    """dash_check_states over every system of the copied words on `threads` host threads (numpy and
    the library call release the interpreter lock). Returns the records, uint32 [nsys, 4]."""
    fn = dash.lib().dash_check_states
    fn.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    rec = np.zeros((nsys, 4), np.uint32)
    per = N * (16 + CS)

    def part(k):
        lo, hi = nsys * k // threads, nsys * (k + 1) // threads
        for a in range(lo, hi, 1 << 14):
            b = min(hi, a + (1 << 14))
            nodes = unpack(words[a * per:b * per], N, CS)
            src, dst = nodes.ctypes.data, rec[a:b].ctypes.data
            for s in range(b - a):
                if fn(src + s * N * NODE_DTYPE.itemsize, N, CS, dst + s * 16, None) != 0:
                    raise RuntimeError("dash_check_states failed")
    with concurrent.futures.ThreadPoolExecutor(threads) as ex:
        list(ex.map(part, range(threads)))
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--systems", type=int, default=1 << 20)
    ap.add_argument("--len", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sample", type=int, default=64, help="systems whose real states fill the old route's buffer")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--kernel-only", action="store_true",
                    help="stop after (a) and write nothing: the program of a counter run (rocprofv3 --pmc)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "coherence.json"))
    args = ap.parse_args()
    assert args.reps >= 7, "the median of at least seven runs"
    import torch
    dash = load_package()
    N, CS, n, L = 8, 4, args.systems, args.len
    torch.cuda.set_device(args.device)
    box = dash.probe_box(args.device)
    out = {"tool": "tools/coherence_row.py",
           "workload": f"{n} systems x {N} nodes x {L} uniform RD/WR per node, CACHE_SIZE {CS}, device generator, "
                       f"lockstep, DASH_KEEP_STATE",
           "systems": n, "box": box, "reps": args.reps, "warmup": args.warmup}
    state_bytes = n * N * (16 + CS) * 4
    sample_n = min(args.sample, n)
    with dash.Engine(n, num_procs=N, cache_size=CS, max_instr=L, device=args.device, keep_state=True) as eng:
        eng.generate(GEN_SEED, L, kind=dash.GEN_UNIFORM)
        stats = eng.run()
        stream = torch.cuda.ExternalStream(eng.stream(), device=args.device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for k in range(args.warmup + args.reps):
            e0.record(stream)
            tot = eng.check_coherence()  # returns with the stream synchronised
            e1.record(stream)
            e1.synchronize()
            if k >= args.warmup:
                ms.append(e0.elapsed_time(e1))
        assert tot["systems"] == n
        k_ms = statistics.median(ms)
        out["kernel"] = {"what": "dash_check_coherence between device events on the handle's stream",
                         "ms": spread(ms), "state_bytes_read": state_bytes, "bytes_per_s": state_bytes / (k_ms * 1e-3),
                         "fraction_of_hbm_peak": state_bytes / (k_ms * 1e-3) / HBM_PEAK, "hbm_peak_bytes_per_s": HBM_PEAK,
                         "kernel_ms_of_the_run": stats["kernel_ms"], "totals": tot}
        out["result"] = {"err_systems": stats["err_systems"], "violating_systems": tot["violating_systems"],
                         "violating_clean_systems": tot["violating_clean_systems"],
                         "violating_clean_share": tot["violating_clean_systems"] / n,
                         "bit_names": list(dash.COH_NAMES), "bit_systems": tot["bit_systems"]}
        print(json.dumps({"kernel_ms": k_ms, "fraction_of_hbm_peak": out["kernel"]["fraction_of_hbm_peak"],
                          "violating_clean_share": out["result"]["violating_clean_share"]}), flush=True)
        if args.kernel_only:
            return 0
        sample = np.concatenate([words_of(eng.read_state(s), CS) for s in range(sample_n)])
        kernel_rec = eng.read_coherence(0, sample_n)
    # (b) the old route: the same number of bytes to pinned host memory, then 16 host threads
    words = state_bytes // 4
    dev = torch.from_numpy(np.resize(sample, words).view(np.int32)).to(f"cuda:{args.device}")
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
    pass_s = []
    for _ in range(3):
        t0 = time.perf_counter()
        rec = host_pass(dash, view, n, N, CS)
        pass_s.append(time.perf_counter() - t0)
    for f, col in zip(("bits", "addrs", "first_addr", "first_bits"), rec[:sample_n].T):
        assert np.array_equal(col, kernel_rec[f]), f  # the host route and the kernel agree on real states
    c_ms = statistics.median(copy_ms)
    out["old_route"] = {"what": "device-to-host copy of state_bytes_read bytes into pinned memory (device events), then "
                                "a 16-thread host pass: numpy unpack into dash_node_state, dash_check_states per system "
                                "(host clock)",
                        "source_buffer": f"state words of the first {sample_n} systems, repeated",
                        "copy_ms": spread(copy_ms), "copy_bytes_per_s": state_bytes / (c_ms * 1e-3),
                        "host_pass_s": spread(pass_s), "host_threads": 16,
                        "host_pass_violating_systems": int((rec[:, 0] != 0).sum())}
    out["kernel_over_copy_alone"] = k_ms / c_ms
    out["kernel_beats_the_copy_alone"] = bool(k_ms < c_ms)
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({"coherence_row": "ok" if out["kernel_beats_the_copy_alone"] else "KERNEL SLOWER THAN THE COPY",
                      "kernel_ms": k_ms, "copy_ms": c_ms, "host_pass_s": statistics.median(pass_s), "out": args.out}))
    return 0 if out["kernel_beats_the_copy_alone"] else 1


if __name__ == "__main__":
    sys.exit(main())
