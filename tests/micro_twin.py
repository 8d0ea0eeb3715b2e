"""CPU twin of the seeded micro-step schedule (dash_set_micro_seeds), for small systems.

TEST INFRASTRUCTURE. The oracle's STRICT model exports no enabled set, so the twin derives it: a
node is enabled after a prefix of steps exactly when oc.replay_steps(prefix + [SEND | POP | ISSUE
of that node]) accepts one of the three (a node holding sends can only send; a node with a message
pops before it issues, as the engine's step does). walk() repeats: enabled set, dash_micro_pick,
append the accepted step, until nothing is enabled. Every probe replays the prefix from the start:
O(steps^2 * 3N) oracle steps, about 0.1 s for tests/golden/reference/test_4.
"""
import numpy as np

import oracle_ctypes as oc
from conftest import load_dash

XK_POP, XK_ISSUE, XK_SEND = 0, 1, 2
ORC_ERR_OVERFLOW = 1  # a queue of the micro-step model (40 messages) overflowed


def enabled_steps(tr, lens, prefix, N, CS):
    """{node: the step word it would take} after `prefix`."""
    out = {}
    for t in range(N):
        for kind in (XK_SEND, XK_POP, XK_ISSUE):
            w = (kind << 8) | t
            try:
                oc.replay_steps(tr, lens, prefix + [w], num_procs=N, cache_size=CS)
            except ValueError:
                continue
            out[t] = w
            break
    return out


def walk(tr, lens, seed, weights, N, CS, max_steps=1 << 14, count_msgs=False):
    """The seeded micro-step schedule (seed, weights) of one system in the STRICT model:
    (witness steps, outcome, terminal). count_msgs: the outcome carries the handled-message counts
    and its digest is folded with them (oc.outcome_key)."""
    dash = load_dash()
    w = dash.pack_weights(weights)
    steps = []
    while len(steps) < max_steps:
        en = enabled_steps(tr, lens, steps, N, CS)
        if not en:
            break
        mask = sum(1 << t for t in en)
        steps.append(en[dash.micro_pick(seed, len(steps), mask, w, N)])
    out, term = oc.replay_steps(tr, lens, steps, num_procs=N, cache_size=CS, count_msgs=count_msgs)
    return steps, out, term


def acts_of(steps, N):
    """A witness as a dash_set_micro_schedule table."""
    acts = np.full((len(steps), N), 0xFF, np.uint8)
    for r, s in enumerate(steps):
        acts[r, s & 15] = 1 if (s >> 8) == XK_SEND else 0
    return acts


def steps_of(acts, events):
    """An engine run's acts (read_micro_acts) and event list as a witness: a delivery is a SEND, a
    step a POP or an ISSUE by the kind of the event it logged."""
    kind = {(e.round, e.node): (XK_ISSUE if e.kind == 1 else XK_POP) for e in events}
    steps = []
    for r, row in enumerate(np.asarray(acts)):
        (t,) = np.nonzero(row != 0xFF)[0].tolist()
        steps.append(((XK_SEND if row[t] == 1 else kind[(r, t)]) << 8) | t)
    return steps
