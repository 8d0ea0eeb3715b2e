"""The per-address sharing profile of include/dash.h (dash_addr_metrics) in plain Python: the reference
the device kernel (csrc/dash_addr.hip) and the host function (dash_addr_metrics_from_events) are
compared with, itself pinned on hand-written event lists (test_addr_metrics_spec.py).

An address is a = (home << 4) | block, a < A = num_procs * 16: bits 14:8 of an event's word, for
instructions and popped messages alike. Every field is a sum or an OR over the events of rounds
[0, K) whose address is a:

    reads, writes           instruction events, by bit 15 of the instruction (set = WR)
    read_misses, write_misses, upgrades
                            READ_REQUEST / WRITE_REQUEST / UPGRADE message events, whoever pops them
    invalidations           INV popped, at any node
    interventions           WRITEBACK_INV + WRITEBACK_INT popped
    flushes                 FLUSH + FLUSH_INVACK popped
    evict_shared, evict_modified
                            EVICT_SHARED / EVICT_MODIFIED popped at the home (node == a >> 4)
    msgs                    every message event
    nodes                   readers | writers << 8 | invalidated << 16, one bit per node that issued an
                            RD / issued a WR / popped an INV

An event whose address is >= A belongs to no record and is counted as foreign.
"""
from metrics_ref import (EVICT_MODIFIED, EVICT_SHARED, FLUSH, FLUSH_INVACK, INV, KIND_INSTR, READ_REQUEST, UPGRADE,
                         WRITE_REQUEST, WRITEBACK_INT, WRITEBACK_INV, msg_word)  # noqa: F401 (msg_word: re-exported)

FIELDS = ("reads", "writes", "read_misses", "write_misses", "upgrades", "invalidations", "interventions", "flushes",
          "evict_shared", "evict_modified", "msgs", "nodes")
SUM_FIELDS = FIELDS[:11]
UNTOUCHED, PRIVATE, READ_SHARED, ONE_WRITER, MULTI_WRITER = range(5)

_BY_TYPE = {READ_REQUEST: "read_misses", WRITE_REQUEST: "write_misses", UPGRADE: "upgrades", INV: "invalidations",
            WRITEBACK_INV: "interventions", WRITEBACK_INT: "interventions", FLUSH: "flushes", FLUSH_INVACK: "flushes"}


def addr_metrics_from_events(events, rounds, num_procs):
    """events: (round, node, kind, word) tuples in any order; rounds: K, the kept rounds. Returns (one
    dict of FIELDS per address, the foreign events)."""
    A = num_procs * 16
    out = [dict.fromkeys(FIELDS, 0) for _ in range(A)]
    foreign = 0
    for rnd, t, kind, word in events:
        if rnd >= rounds:
            continue
        a = (word >> 8) & 0x7F
        if a >= A:
            foreign += 1
            continue
        m = out[a]
        if kind == KIND_INSTR:
            wr = bool(word & 0x8000)
            m["writes" if wr else "reads"] += 1
            m["nodes"] |= 1 << (t + (8 if wr else 0))
            continue
        mtype = word & 15
        m["msgs"] += 1
        if mtype in _BY_TYPE:
            m[_BY_TYPE[mtype]] += 1
        if mtype == INV:
            m["nodes"] |= 1 << (16 + t)
        if mtype in (EVICT_SHARED, EVICT_MODIFIED) and t == a >> 4:
            m["evict_shared" if mtype == EVICT_SHARED else "evict_modified"] += 1
    return out, foreign


def addr_class(m):
    """The class of a record, as include/dash.h defines DASH_ADDR_*."""
    r, w = m["nodes"] & 0xFF, (m["nodes"] >> 8) & 0xFF
    nodes, writers = bin(r | w).count("1"), bin(w).count("1")
    if m["reads"] + m["writes"] == 0:
        return UNTOUCHED
    if nodes == 1:
        return PRIVATE
    if w == 0 and nodes >= 2:
        return READ_SHARED
    if writers == 1 and nodes >= 2:
        return ONE_WRITER
    assert writers >= 2
    return MULTI_WRITER


def totals_from_records(systems):
    """dash_addr_totals' sums and class counts from the records of a batch: systems is a list of
    per-address dict lists."""
    tot = dict.fromkeys(SUM_FIELDS, 0)
    tot.update(msgs_max=0, class_addrs=[0] * 5, class_misses=[0] * 5, class_invalidations=[0] * 5)
    for recs in systems:
        for m in recs:
            for f in SUM_FIELDS:
                tot[f] += m[f]
            tot["msgs_max"] = max(tot["msgs_max"], m["msgs"])
            c = addr_class(m)
            tot["class_addrs"][c] += 1
            tot["class_misses"][c] += m["read_misses"] + m["write_misses"] + m["upgrades"]
            tot["class_invalidations"][c] += m["invalidations"]
    return tot
