"""The per-address definitions of include/dash.h as tests/addr_metrics_ref.py states them, pinned without
the device: hand-written event lists that each isolate one rule, the full truth table of
dash_addr_class, and libdash.so's host function (dash_addr_metrics_from_events) against the Python
reference and the per-node reference on the oracle's own text logs of the five reference fixtures."""
import itertools

import pytest

import addr_metrics_ref as ar
import metrics_ref as mr
import oracle_ctypes as oc
from metrics_ref import KIND_INSTR as I, KIND_MSG as M, msg_word

RD, WR = 0x0000, 0x8000  # instruction words: bit 15 = WR
FIXTURES = ["sample", "test_1", "test_2", "test_3", "test_4"]


def instr(kind, address, value=0):
    return kind | address << 8 | value


def nonzero(m):
    return {k: v for k, v in m.items() if v}


def touched(records):
    return {a: nonzero(m) for a, m in enumerate(records) if nonzero(m)}


def as_dicts(rec):
    return [{f: int(m[f]) for f in ar.FIELDS} for m in rec]


def both(dash, events, rounds, num_procs):
    """The Python reference's records and foreign count, checked equal to the host function's."""
    want, foreign = ar.addr_metrics_from_events(events, rounds, num_procs)
    rec, got_foreign = dash.addr_metrics_from_events(events, num_procs, rounds)
    assert rec.dtype.names == ar.FIELDS == dash.ADDR_METRIC_FIELDS and rec.shape == (num_procs * 16,)
    assert as_dicts(rec) == want and got_foreign == foreign
    return want, foreign


def test_a_request_counts_at_its_address_whoever_pops_it(dash):
    # three requests on 0x10: popped at the home (node 1) and, as no protocol run would, at node 3
    ev = [(0, 1, M, msg_word(mr.READ_REQUEST, 2, 0x10)), (1, 3, M, msg_word(mr.WRITE_REQUEST, 0, 0x10)),
          (2, 1, M, msg_word(mr.UPGRADE, 3, 0x10)), (3, 0, M, msg_word(mr.READ_REQUEST, 1, 0x05))]
    rec, foreign = both(dash, ev, 4, 4)
    assert touched(rec) == {0x10: {"read_misses": 1, "write_misses": 1, "upgrades": 1, "msgs": 3},
                            0x05: {"read_misses": 1, "msgs": 1}}
    assert foreign == 0


def test_instructions_set_the_reader_and_writer_bits(dash):
    ev = [(0, 0, I, instr(RD, 0x21)), (0, 2, I, instr(RD, 0x21)), (1, 2, I, instr(WR, 0x21, 7)),
          (2, 3, I, instr(WR, 0x3F, 9)), (5, 2, I, instr(RD, 0x21))]
    rec, _ = both(dash, ev, 6, 4)
    assert touched(rec) == {0x21: {"reads": 3, "writes": 1, "nodes": 0b0101 | 0b0100 << 8},
                            0x3F: {"writes": 1, "nodes": 0b1000 << 8}}


def test_the_forwarded_evict_shared_is_a_message_but_no_eviction(dash):
    # node 2 evicts a shared line homed on node 1 (address 0x13); the home forwards EVICT_SHARED to the
    # last sharer, node 0: that one is popped away from the home
    ev = [(0, 1, M, msg_word(mr.EVICT_SHARED, 2, 0x13)), (1, 0, M, msg_word(mr.EVICT_SHARED, 1, 0x13)),
          (2, 1, M, msg_word(mr.EVICT_MODIFIED, 3, 0x14)), (3, 2, M, msg_word(mr.EVICT_MODIFIED, 3, 0x14))]
    rec, _ = both(dash, ev, 4, 4)
    assert touched(rec) == {0x13: {"evict_shared": 1, "msgs": 2}, 0x14: {"evict_modified": 1, "msgs": 2}}


def test_inv_sets_invalidated_for_the_node_that_pops_it(dash):
    ev = [(0, 3, M, msg_word(mr.INV, 1, 0x10)), (1, 0, M, msg_word(mr.INV, 1, 0x10)), (2, 3, M, msg_word(mr.INV, 1, 0x10)),
          (3, 2, M, msg_word(mr.WRITEBACK_INV, 1, 0x10)), (4, 2, M, msg_word(mr.WRITEBACK_INT, 1, 0x11)),
          (5, 1, M, msg_word(mr.FLUSH, 2, 0x10)), (6, 0, M, msg_word(mr.FLUSH_INVACK, 2, 0x10))]
    rec, _ = both(dash, ev, 7, 4)
    assert touched(rec) == {0x10: {"invalidations": 3, "interventions": 1, "flushes": 2, "msgs": 6, "nodes": 0b1001 << 16},
                            0x11: {"interventions": 1, "msgs": 1}}


def test_replies_count_in_msgs_only(dash):
    ev = [(r, 0, M, msg_word(t, 1, 0x02)) for r, t in enumerate((mr.REPLY_RD, mr.REPLY_WR, mr.REPLY_ID))]
    rec, _ = both(dash, ev, 3, 2)
    assert touched(rec) == {0x02: {"msgs": 3}}


def test_events_at_or_past_the_kept_rounds_are_dropped(dash):
    ev = [(0, 0, I, instr(RD, 0x01)), (3, 1, M, msg_word(mr.INV, 0, 0x01)), (4, 1, I, instr(WR, 0x01, 1)),
          (9, 0, M, msg_word(mr.READ_REQUEST, 1, 0x01))]
    whole, _ = both(dash, ev, 10, 2)
    assert touched(whole) == {0x01: {"reads": 1, "writes": 1, "read_misses": 1, "invalidations": 1, "msgs": 2,
                                     "nodes": 0b01 | 0b10 << 8 | 0b10 << 16}}
    cut, _ = both(dash, ev, 4, 2)  # K = 4: rounds 4 and 9 lie past the kept rounds
    assert touched(cut) == {0x01: {"reads": 1, "invalidations": 1, "msgs": 1, "nodes": 0b01 | 0b10 << 16}}
    assert touched(both(dash, ev, 0, 2)[0]) == {}


def test_an_address_past_the_systems_last_goes_to_foreign_and_to_no_record(dash):
    # 3 nodes: A = 48; 0x30 and 0x7F name homes the system does not have
    ev = [(0, 0, I, instr(RD, 0x2F)), (1, 1, I, instr(WR, 0x30, 1)), (2, 2, M, msg_word(mr.INV, 0, 0x7F)),
          (3, 2, I, instr(RD, 0x30)), (7, 1, I, instr(RD, 0x7F))]
    rec, foreign = both(dash, ev, 7, 3)
    assert touched(rec) == {0x2F: {"reads": 1, "nodes": 0b001}} and foreign == 3 and len(rec) == 48


def record(r, w):
    """A record whose counts agree with its reader and writer sets."""
    return dict.fromkeys(ar.FIELDS, 0) | {"reads": bin(r).count("1"), "writes": 2 * bin(w).count("1"), "nodes": r | w << 8}


def test_the_truth_table_of_dash_addr_class(dash):
    seen = set()
    for r, w in itertools.product(range(8), repeat=2):  # every (readers, writers) pair of 3 nodes
        m = record(r, w)
        both_sets, writers = bin(r | w).count("1"), bin(w).count("1")
        want = (ar.UNTOUCHED if r | w == 0 else ar.PRIVATE if both_sets == 1 else ar.MULTI_WRITER if writers >= 2
                else ar.ONE_WRITER if writers == 1 else ar.READ_SHARED)
        assert ar.addr_class(m) == want and dash.addr_class(m) == want, (r, w)
        # neither the invalidated byte nor the message fields decide anything
        assert dash.addr_class(m | {"nodes": m["nodes"] | 0xFF << 16, "msgs": 9, "invalidations": 9}) == want
        seen.add(want)
    assert seen == {0, 1, 2, 3, 4}
    assert (dash.ADDR_UNTOUCHED, dash.ADDR_PRIVATE, dash.ADDR_READ_SHARED, dash.ADDR_ONE_WRITER,
            dash.ADDR_MULTI_WRITER) == (0, 1, 2, 3, 4)
    empty = dict.fromkeys(ar.FIELDS, 0)
    assert dash.addr_class(empty) == ar.addr_class(empty) == ar.UNTOUCHED
    # messages alone touch nothing: an address only ever invalidated at a node that never used it
    assert dash.addr_class(empty | {"msgs": 2, "invalidations": 2, "nodes": 0b11 << 16}) == ar.UNTOUCHED


@pytest.mark.parametrize("test", FIXTURES)
def test_host_function_on_the_oracles_text_log(dash, test):
    tr, lens = oc.load_test_dir(oc.GOLDEN / test)
    res, log = oc.run_system(tr, lens, num_procs=4, cache_size=4, log=True, log_msgs=True)
    assert res.errors == 0
    ev = mr.events_from_text(log)
    assert len(ev) == len(log.splitlines()) > 0
    rec, foreign = both(dash, ev, len(ev), 4)
    assert foreign == 0
    # the other axis of the same log: sums over addresses == sums over nodes
    nodes = mr.metrics_from_events(ev, len(ev), 4)
    for f in ("read_misses", "write_misses", "upgrades", "invalidations", "interventions", "evict_shared",
              "evict_modified", "msgs", "reads", "writes"):
        assert sum(m[f] for m in rec) == mr.total(nodes, f), f
    hist = list(res.hist)
    assert sum(m["flushes"] for m in rec) == hist[mr.FLUSH] + hist[mr.FLUSH_INVACK]
    assert sum(m["msgs"] for m in rec) == sum(hist)
    # an address's reader and writer sets are the nodes whose traces name it
    for a, m in enumerate(rec):
        readers = sum(1 << t for t in range(4) if any((w >> 8) & 0x7F == a and not w & 0x8000 for w in tr[t][:lens[t]]))
        writers = sum(1 << t for t in range(4) if any((w >> 8) & 0x7F == a and w & 0x8000 for w in tr[t][:lens[t]]))
        assert m["nodes"] & 0xFFFF == readers | writers << 8, a
    # half the log: the cut applies to every field
    half, _ = both(dash, ev, len(ev) // 2, 4)
    assert sum(m["reads"] + m["writes"] + m["msgs"] for m in half) == len(ev) // 2


def test_einval(dash):
    import ctypes
    L = dash.lib()
    out = (dash.AddrMetrics * 128)()
    ev = (dash.Event * 1)()
    assert L.dash_addr_metrics_from_events(ev, 1, 0, 4, out, None) == dash.EINVAL
    assert L.dash_addr_metrics_from_events(ev, 1, 9, 4, out, None) == dash.EINVAL
    assert L.dash_addr_metrics_from_events(ev, 1, 4, 4, None, None) == dash.EINVAL
    assert L.dash_addr_metrics_from_events(None, 1, 4, 4, out, None) == dash.EINVAL
    assert L.dash_addr_metrics_from_events(None, 0, 4, 4, out, None) == dash.OK   # no events: all-zero records
    assert L.dash_addr_metrics_from_events(ev, 1, 8, 4, out, None) == dash.OK     # foreign is optional
    assert L.dash_addr_class(None) == dash.EINVAL
    assert ctypes.sizeof(dash.AddrMetrics) == 48 and ctypes.sizeof(dash.AddrTotals) == 30 * 8
    for name in ("dash_compute_addr_metrics", "dash_read_addr_metrics", "dash_addr_class", "dash_addr_metrics_from_events"):
        assert name in dash.EXPORTS
