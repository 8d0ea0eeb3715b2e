"""The metric definitions of include/dash.h as tests/metrics_ref.py states them, pinned without the
engine: hand-written event lists that each isolate one rule, and the oracle's own text logs of
the five reference fixtures against the oracle's message histogram."""
import pytest

import metrics_ref as mr
import oracle_ctypes as oc
from metrics_ref import KIND_INSTR as I, KIND_MSG as M, metrics_from_events, msg_word

RD, WR = 0x0000, 0x8000  # instruction words: bit 15 = WR


def nonzero(m):
    return {k: v for k, v in m.items() if v and k != "idle_rounds"}


def test_requests_count_for_their_sender_not_for_the_home():
    ev = [(0, 2, I, RD | 0x10 << 8), (1, 1, M, msg_word(mr.READ_REQUEST, 2, 0x10)),
          (2, 3, I, WR | 0x10 << 8 | 7), (3, 1, M, msg_word(mr.WRITE_REQUEST, 3, 0x10)),
          (4, 0, I, WR | 0x10 << 8 | 9), (5, 1, M, msg_word(mr.UPGRADE, 0, 0x10))]
    m = metrics_from_events(ev, 8, 4)
    assert nonzero(m[1]) == {"msgs": 3, "home_requests": 3}  # the directory's load, none of its own
    assert nonzero(m[2]) == {"reads": 1, "read_misses": 1}
    assert nonzero(m[3]) == {"writes": 1, "write_misses": 1}
    assert nonzero(m[0]) == {"writes": 1, "upgrades": 1}


def test_invalidations_and_interventions_count_for_the_node_that_pops_them():
    ev = [(0, 3, M, msg_word(mr.INV, 1, 0x10)), (1, 2, M, msg_word(mr.WRITEBACK_INV, 1, 0x10)),
          (2, 2, M, msg_word(mr.WRITEBACK_INT, 1, 0x10))]
    m = metrics_from_events(ev, 3, 4)
    assert nonzero(m[3]) == {"msgs": 1, "invalidations": 1}
    assert nonzero(m[2]) == {"msgs": 2, "interventions": 2}
    assert nonzero(m[1]) == {}


def test_evict_shared_counts_at_the_home_and_the_forwarded_one_does_not():
    # node 2 evicts a shared line homed on node 1 (address 0x13); the home forwards EVICT_SHARED
    # to the last sharer, node 0, with itself as the sender: that one is no eviction of node 1's
    ev = [(0, 1, M, msg_word(mr.EVICT_SHARED, 2, 0x13)), (1, 0, M, msg_word(mr.EVICT_SHARED, 1, 0x13)),
          (2, 1, M, msg_word(mr.EVICT_MODIFIED, 3, 0x14))]
    m = metrics_from_events(ev, 3, 4)
    assert nonzero(m[2]) == {"evict_shared": 1}
    assert nonzero(m[3]) == {"evict_modified": 1}
    assert nonzero(m[1]) == {"msgs": 2}
    assert nonzero(m[0]) == {"msgs": 1}


def test_a_wait_is_closed_by_any_completing_pop_also_a_stray_flush():
    # node 0 issues at round 2; a FLUSH of another transaction reaches it at round 5 and clears
    # waitingForReply; the REPLY_RD at round 9 then finds no open span
    ev = [(2, 0, I, RD | 0x10 << 8), (5, 0, M, msg_word(mr.FLUSH, 3, 0x01)), (9, 0, M, msg_word(mr.REPLY_RD, 1, 0x10))]
    m = metrics_from_events(ev, 12, 2)[0]
    assert (m["waits"], m["wait_rounds"], m["wait_max"]) == (1, 3, 3)
    for closer, span in ((mr.REPLY_RD, 1), (mr.REPLY_WR, 2), (mr.REPLY_ID, 3), (mr.FLUSH_INVACK, 4)):
        ev = [(10, 1, I, WR | 0x05 << 8), (10 + span, 1, M, msg_word(closer, 0, 0x05))]
        m = metrics_from_events(ev, 20, 2)[1]
        assert (m["waits"], m["wait_rounds"], m["wait_max"]) == (1, span, span)
    for other in (mr.READ_REQUEST, mr.WRITE_REQUEST, mr.INV, mr.UPGRADE, mr.WRITEBACK_INV, mr.WRITEBACK_INT,
                  mr.EVICT_SHARED, mr.EVICT_MODIFIED):
        ev = [(0, 1, I, RD | 0x05 << 8), (3, 1, M, msg_word(other, 0, 0x05))]
        assert metrics_from_events(ev, 20, 2)[1]["waits"] == 0


def test_wait_sum_and_maximum_over_several_spans():
    ev = [(0, 0, I, RD), (4, 0, M, msg_word(mr.REPLY_RD, 1, 0)), (5, 0, I, WR), (7, 0, M, msg_word(mr.REPLY_ID, 1, 0)),
          (8, 0, I, RD), (9, 0, M, msg_word(mr.REPLY_RD, 1, 0))]
    m = metrics_from_events(ev, 10, 2)[0]
    assert (m["waits"], m["wait_rounds"], m["wait_max"]) == (3, 4 + 2 + 1, 4)


def test_a_completing_pop_after_the_next_instruction_belongs_to_that_instruction():
    # a hit at round 1 (no reply), the next instruction at round 2, its reply at round 6: one span,
    # counted from round 2
    ev = [(1, 0, I, RD), (2, 0, I, WR), (6, 0, M, msg_word(mr.REPLY_WR, 1, 0))]
    m = metrics_from_events(ev, 8, 2)[0]
    assert (m["waits"], m["wait_rounds"], m["wait_max"]) == (1, 4, 4)


def test_a_span_open_at_the_cut_is_not_counted():
    ev = [(1, 0, I, RD), (3, 0, M, msg_word(mr.REPLY_RD, 1, 0)), (4, 0, I, RD), (9, 0, M, msg_word(mr.REPLY_RD, 1, 0))]
    whole = metrics_from_events(ev, 10, 2)[0]
    cut = metrics_from_events(ev, 9, 2)[0]  # K = 9: the second reply lies past the kept rounds
    assert (whole["waits"], whole["wait_rounds"], whole["wait_max"]) == (2, 7, 5)
    assert (cut["waits"], cut["wait_rounds"], cut["wait_max"]) == (1, 2, 2)
    assert (cut["reads"], cut["msgs"]) == (2, 1)
    assert metrics_from_events(ev, 0, 2) == [dict.fromkeys(mr.FIELDS, 0)] * 2


def test_idle_rounds_identity():
    ev = [(0, 0, I, RD), (1, 1, M, msg_word(mr.READ_REQUEST, 0, 0x10)), (3, 0, M, msg_word(mr.REPLY_RD, 1, 0x10))]
    deliveries = [(2, 1), (4, 1), (11, 0)]  # the last one lies past K
    m = metrics_from_events(ev, 10, 3, deliveries)
    assert [x["deliveries"] for x in m] == [0, 2, 0]
    assert [x["idle_rounds"] for x in m] == [10 - 2, 10 - 1 - 2, 10]
    for x in m:
        assert x["idle_rounds"] == 10 - (x["reads"] + x["writes"] + x["msgs"]) - x["deliveries"]


@pytest.mark.parametrize("test", ["sample", "test_1", "test_2", "test_3", "test_4"])
def test_counts_from_the_oracles_text_log_add_up_to_its_histogram(test):
    tr, lens = oc.load_test_dir(oc.GOLDEN / test)
    res, log = oc.run_system(tr, lens, num_procs=4, cache_size=4, log=True, log_msgs=True)
    assert res.errors == 0
    ev = mr.events_from_text(log)
    assert len(ev) == len(log.splitlines())
    m = metrics_from_events(ev, len(ev), 4)
    hist = list(res.hist)
    assert mr.total(m, "read_misses") == hist[mr.READ_REQUEST]
    assert mr.total(m, "write_misses") == hist[mr.WRITE_REQUEST]
    assert mr.total(m, "upgrades") == hist[mr.UPGRADE]
    assert mr.total(m, "invalidations") == hist[mr.INV]
    assert mr.total(m, "interventions") == hist[mr.WRITEBACK_INV] + hist[mr.WRITEBACK_INT]
    assert mr.total(m, "msgs") == sum(hist)
    assert mr.total(m, "home_requests") == hist[mr.READ_REQUEST] + hist[mr.WRITE_REQUEST] + hist[mr.UPGRADE]
    assert mr.total(m, "reads") + mr.total(m, "writes") == res.instructions
    # per node: what it issued is its trace, and it cannot miss more often than it issued
    for t in range(4):
        assert m[t]["reads"] + m[t]["writes"] == lens[t]
        assert m[t]["read_misses"] <= m[t]["reads"]
        assert m[t]["write_misses"] + m[t]["upgrades"] <= m[t]["writes"]
