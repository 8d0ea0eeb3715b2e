"""The per-node metrics of include/dash.h (dash_node_metrics) in plain Python: the reference the
device kernel (csrc/dash_metrics.hip) is compared with, itself pinned on hand-written event lists
and on the oracle's text logs (test_metrics_spec.py).

All metrics are pure functions of one system's event log over its kept rounds [0, K):

    reads, writes           instruction events of node t, by bit 15 of the instruction (set = WR)
    read_misses, write_misses, upgrades
                            READ_REQUEST / WRITE_REQUEST / UPGRADE message events at any node whose
                            sender is t (requests are only popped at the home: t's serviced requests)
    msgs                    message events popped by t
    home_requests           READ_REQUEST + WRITE_REQUEST + UPGRADE popped by t
    invalidations           INV popped by t
    interventions           WRITEBACK_INV + WRITEBACK_INT popped by t
    evict_shared, evict_modified
                            EVICT_SHARED / EVICT_MODIFIED events with sender t popped at node
                            address >> 4 (not the home's forwarded EVICT_SHARED, popped elsewhere)
    waits, wait_rounds, wait_max
                            for each instruction event of t at round r0: t's next event of a completing
                            type (REPLY_RD, REPLY_WR, REPLY_ID, FLUSH, FLUSH_INVACK), at round r1, if
                            it comes before t's next instruction event, gives the span r1 - r0: their
                            count, sum and maximum. A span still open at round K is not counted
    deliveries              delivery markers of node t (seeded micro-step schedules only)
    idle_rounds             K - (reads + writes + msgs) - deliveries
"""
FIELDS = ("reads", "writes", "read_misses", "write_misses", "upgrades", "msgs", "home_requests",
          "invalidations", "interventions", "evict_shared", "evict_modified", "waits", "wait_rounds",
          "wait_max", "deliveries", "idle_rounds")
# the fields that need no round numbers, only each node's own event order: what a text log gives
COUNT_FIELDS = FIELDS[:11] + ("waits",)

KIND_MSG, KIND_INSTR = 0, 1  # DASH_EV_MSG, DASH_EV_INSTR
(READ_REQUEST, WRITE_REQUEST, REPLY_RD, REPLY_WR, REPLY_ID, INV, UPGRADE, WRITEBACK_INV, WRITEBACK_INT,
 FLUSH, FLUSH_INVACK, EVICT_SHARED, EVICT_MODIFIED) = range(13)
COMPLETING = (REPLY_RD, REPLY_WR, REPLY_ID, FLUSH, FLUSH_INVACK)


def msg_word(mtype, sender, address):
    """A message event's word as dash_event.word documents it: type[3:0], sender[6:4], address[14:8]."""
    return mtype | (sender << 4) | (address << 8)


def metrics_from_events(events, rounds, num_procs, deliveries=()):
    """events: (round, node, kind, word) tuples, at most one per node and round; deliveries: (round,
    node) delivery markers; rounds: K, the kept rounds. Anything at a round >= K is ignored.
    Returns one dict of FIELDS per node."""
    out = [dict.fromkeys(FIELDS, 0) for _ in range(num_procs)]
    issued = [None] * num_procs  # round of the node's last instruction while its span is open
    for rnd, t, kind, word in sorted(events, key=lambda e: (e[0], e[1])):
        if rnd >= rounds:
            continue
        m = out[t]
        if kind == KIND_INSTR:
            m["writes" if word & 0x8000 else "reads"] += 1
            issued[t] = rnd
            continue
        mtype, sender, address = word & 15, (word >> 4) & 7, (word >> 8) & 0x7F
        m["msgs"] += 1
        if mtype in (READ_REQUEST, WRITE_REQUEST, UPGRADE):
            m["home_requests"] += 1
            if sender < num_procs:
                out[sender][{READ_REQUEST: "read_misses", WRITE_REQUEST: "write_misses",
                             UPGRADE: "upgrades"}[mtype]] += 1
        if mtype == INV:
            m["invalidations"] += 1
        if mtype in (WRITEBACK_INV, WRITEBACK_INT):
            m["interventions"] += 1
        if mtype in (EVICT_SHARED, EVICT_MODIFIED) and address >> 4 == t and sender < num_procs:
            out[sender]["evict_shared" if mtype == EVICT_SHARED else "evict_modified"] += 1
        if mtype in COMPLETING:
            if issued[t] is not None:
                span = rnd - issued[t]
                m["waits"] += 1
                m["wait_rounds"] += span
                m["wait_max"] = max(m["wait_max"], span)
            issued[t] = None
    for rnd, t in deliveries:
        if rnd < rounds:
            out[t]["deliveries"] += 1
    for m in out:
        m["idle_rounds"] = rounds - (m["reads"] + m["writes"] + m["msgs"]) - m["deliveries"]
    return out


def events_from_text(text):
    """The DEBUG_MSG / DEBUG_INSTR lines of a run (the oracle's, the reference's, or
    dash.format_events') as event tuples whose "round" is the line number: each node's own order is
    kept, so COUNT_FIELDS of metrics_from_events(events, len(events), N) are the run's."""
    import oracle_ctypes as oc
    ev = []
    for line in text.splitlines():
        m = oc.LOG_MSG.match(line)
        if m:
            ev.append((len(ev), int(m[1]), KIND_MSG, msg_word(int(m[3]), int(m[2]), int(m[4], 16))))
            continue
        m = oc.LOG_INSTR.match(line)
        if m:
            ev.append((len(ev), int(m[1]), KIND_INSTR, oc.pack(m[2], int(m[3], 16), int(m[4]))))
    return ev


def total(metrics, field):
    return sum(m[field] for m in metrics)
