"""Writes tests/golden/shrink_long.json: the twin's result (tests/shrink_ref.py over the CPU oracle) for
a source of 8 nodes x 600 instructions, the input of the two-x-block test of
tests/test_gpu_launch_edges.py. The twin takes minutes at this length, so its steps, lengths and
traces are committed; tests/test_launch_edges_spec.py re-checks them cheaply.

The source is found, not stored: the first rng seed from 600 on whose batch
(tests/launch_edges.long_source) holds a system that is incoherent with no error bit under the
lockstep schedule and whose twin takes a step on node 6 or 7 while a stream is still written in more
than 1,024 (node, chunk) items.

    python tests/golden/make_shrink_long.py
"""
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import launch_edges as le  # noqa: E402
import shrink_ref as sr  # noqa: E402


def steps_cross(lens, steps):
    """The steps on node 6 or 7 taken while 8 * wchunks > 1,024 (the base's lengths before the step)."""
    ln = [int(x) for x in lens]
    out = []
    for i, (t, _s, n, _c) in enumerate(steps):
        if t >= 6 and le.LONG_N * le.write_chunks(le.LONG_M, max(ln)) > le.VARIANT_ITEMS_PER_BLOCK:
            out.append(i)
        ln[t] -= n
    return out


def main():
    for rng_seed in range(600, 700):
        src = le.long_source(rng_seed)
        if src is None:
            continue
        k, tr, lens, bits = src
        bit = bits & -bits
        print(f"rng {rng_seed}: system {k}, bits 0x{bits:X}, goal 0x{bit:X}", flush=True)
        out_tr, out_ln, steps = sr.shrink(tr, lens, le.LONG_N, le.LONG_CS, 0, (bit, 0, 0xFFFFFFFF))
        if not steps_cross(lens, steps):
            print("  no step on node 6 or 7 above 1,024 items", flush=True)
            continue
        rec = {"rng": rng_seed, "index": int(k), "bit": int(bit),
               "steps": [[int(x) for x in s] for s in steps], "lens": [int(x) for x in out_ln],
               "trace": [[f"{int(w):04x}" for w in out_tr[t, :int(out_ln[t])]] for t in range(le.LONG_N)]}
        body = ",\n".join(f' "{key}": {json.dumps(val)}' for key, val in rec.items())
        le.LONG_FIXTURE.write_text("{\n" + body + "\n}\n")
        print(f"  {len(steps)} steps, {int(lens.sum())} -> {int(out_ln.sum())} instructions: {le.LONG_FIXTURE}")
        return
    raise SystemExit("no source found")


if __name__ == "__main__":
    main()
