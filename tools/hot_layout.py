#!/usr/bin/env python3
"""Code layout of the round loop of the headline kernel (static, CPU only).

Disassembles the gfx950 code object inside libdash.so like tools/isa_table.py and reports, for
sim_kernel<8, 4, 16, 0>, what a wave fetches and branches through on the common path of a trip:

- the hot span: from the loop header to the latch (the first backward branch behind the trip's
  four arrival exchanges), in instructions and bytes;
- every branch inside the span with its direction: `skip` (forward, target inside the span: taken
  whenever the region it guards is empty), `out` (forward, target behind the latch: an
  out-of-line block, not taken on the common path), `inner` (backward, target inside the span:
  the latch of an inner loop), `latch` (back to the header);
- the inner loops that lie inside the span, and the out-of-line blocks that branch back into it.

Usage: python3 tools/hot_layout.py [libdash.so] [kernel-symbol] [--json out.json]
"""
import collections
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_table  # noqa: E402
import kernel_fingerprint  # noqa: E402

ROUNDS_PER_TRIP = isa_table.ROUNDS_PER_TRIP


def is_branch(x):
    return x["op"].startswith("s_cbranch") or x["op"] == "s_branch"


def layout(insns):
    """The round loop's hot span and its branches, from kernel_insns()'s list."""
    xchg = [x["off"] for x in insns if x["op"].startswith("ds_wrxchg")]
    back = [x for x in insns if x["tgt"] is not None and x["tgt"] <= x["off"]]
    # the latch: of the backward branches around one trip's arrival exchanges, the first one.
    # Blocks laid behind the loop branch back into it from further on.
    cands = [x for x in back if sum(x["tgt"] <= o <= x["off"] for o in xchg) >= ROUNDS_PER_TRIP]
    if not cands:
        raise ValueError("no round loop found")
    latch = min(cands, key=lambda x: x["off"])
    lo, hi = latch["tgt"], latch["off"]
    span = [x for x in insns if lo <= x["off"] <= hi]
    end = hi + latch["size"]
    branches = []
    for x in span:
        if not is_branch(x):
            continue
        t = x["tgt"]
        if x is latch or t == lo:
            kind = "latch"
        elif lo < t <= x["off"]:
            kind = "inner"
        elif x["off"] < t <= hi:
            kind = "skip"
        else:
            kind = "out"
        over = sum(1 for y in span if x["off"] < y["off"] < t) if kind == "skip" else None
        branches.append({"off": x["off"] - lo, "op": x["op"], "target": t - lo, "kind": kind, "over": over})
    inner = [[b["target"], b["off"]] for b in branches if b["kind"] == "inner"]
    # out-of-line blocks: code outside the span that branches (back) into it
    reentries = sorted({x["tgt"] - lo for x in insns if is_branch(x) and x["tgt"] is not None
                        and not lo <= x["off"] <= hi and lo < x["tgt"] <= hi})
    cond = [b for b in branches if b["op"] != "s_branch"]
    # what must stay inline shows in the span's memory operations: per round two arrival ORs
    # (ds_or), the ring stores of the two place regions, one arrival exchange; per trip the refill
    mem = collections.Counter(x["op"] for x in span if x["op"].startswith(("ds_", "global_", "buffer_", "flat_")))
    return {"rounds_per_trip": ROUNDS_PER_TRIP,
            "hot_span": {"header": lo, "latch": hi, "instructions": len(span), "bytes": end - lo},
            "memory_ops": dict(sorted(mem.items())),
            "branches": branches,
            "conditional_branches": len(cond),
            "conditional_by_kind": {k: sum(b["kind"] == k for b in cond) for k in ("skip", "out", "inner", "latch")},
            "inner_loops": inner,
            "reentry_points": reentries}


def report(lib, sym):
    rep = layout(isa_table.kernel_insns(isa_table.extract(lib), sym))
    return {"kernel": sym, "kernel_fingerprint": kernel_fingerprint.fingerprint(lib, sym),
            "source": "tools/hot_layout.py (static)", **rep}


def main():
    args = [a for i, a in enumerate(sys.argv[1:], 1) if a != "--json" and sys.argv[i - 1] != "--json"]
    lib = args[0] if args else str(kernel_fingerprint.LIB)
    sym = args[1] if len(args) > 1 else isa_table.SYM
    rep = report(lib, sym)
    h = rep["hot_span"]
    print(f"kernel {sym} ({rep['kernel_fingerprint']})")
    print(f"hot span of the round loop: +0x{h['header']:x}..+0x{h['latch']:x}, {h['instructions']} instructions, "
          f"{h['bytes']} bytes per trip of {ROUNDS_PER_TRIP} rounds "
          f"({h['instructions'] / ROUNDS_PER_TRIP:.1f} instructions, {h['bytes'] / ROUNDS_PER_TRIP:.0f} bytes per round)")
    k = rep["conditional_by_kind"]
    print(f"conditional branches in the span: {rep['conditional_branches']} "
          f"(skip {k['skip']}, out of line {k['out']}, inner-loop latch {k['inner']}, latch {k['latch']})")
    print(f"\n{'offset':>8s}  {'branch':18s} {'kind':6s} target")
    for b in rep["branches"]:
        what = f"+0x{b['target']:x}" + (f" (over {b['over']} instructions)" if b["over"] is not None else "")
        print(f"{'+0x%x' % b['off']:>8s}  {b['op']:18s} {b['kind']:6s} {what}")
    print("\nmemory operations in the span: " + ", ".join(f"{n} {op}" for op, n in rep["memory_ops"].items()))
    print(f"inner loops inside the span: {len(rep['inner_loops'])}"
          + "".join(f"\n  +0x{t:x}..+0x{s:x}" for t, s in rep["inner_loops"]))
    print(f"out-of-line code re-enters the span at {len(rep['reentry_points'])} points"
          + (": " + " ".join(f"+0x{t:x}" for t in rep["reentry_points"]) if rep["reentry_points"] else ""))
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(rep, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
