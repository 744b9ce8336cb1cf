"""The residency of a group's cells as a transition table: which form a cell is in (none, averages, bearers, flows), whether the
form's counters exist on top of it, and what every setter makes of every state.  The table below is pinned as data and walked with
setters and getters alone -- no kernel is launched.  A getter answers exactly in its own state and returns RS_ERR_STATE in every
other; a setter that is refused leaves every getter's answer as it was; counters that a setter keeps are read back with the values
they were given."""
import numpy as np
import pytest

OK, INVALID, STATE = 0, -1, -4  # RS_OK, RS_ERR_INVALID, RS_ERR_STATE
NONE, AVG, AVG_C, BEAR, BEAR_C, FLOWS = "none", "averages", "averages + per-user counters", "bearers", "bearers + counters", "flows"
GETTERS = ("get_avg", "get_avg_counters", "get_bearers", "get_counters", "get_flows")
ANSWERS = {NONE: (), AVG: ("get_avg",), AVG_C: ("get_avg", "get_avg_counters"), BEAR: ("get_bearers",),
           BEAR_C: ("get_bearers", "get_counters"), FLOWS: ("get_flows",)}

# (state, setter) -> (return code, state afterwards, the counters afterwards: "kept" the state's own, "new" the setter's, None: none)
SAME = lambda s, rc: (rc, s, "kept" if s in (AVG_C, BEAR_C) else None)  # noqa: E731 -- a refusal, or a setter that moves nothing
TABLE_9 = {  # RS_SCHED_MAXCELL: averages and bearers
    NONE: dict(set_avg=(OK, AVG, None), set_pending=SAME(NONE, STATE), set_avg_counters=SAME(NONE, STATE),
               set_bearers=(OK, BEAR, None), set_counters=SAME(NONE, STATE), set_flows=SAME(NONE, INVALID)),
    AVG: dict(set_avg=(OK, AVG, None), set_pending=SAME(AVG, OK), set_avg_counters=(OK, AVG_C, "new"),
              set_bearers=(OK, BEAR, None), set_counters=SAME(AVG, STATE), set_flows=SAME(AVG, INVALID)),
    AVG_C: dict(set_avg=(OK, AVG_C, "kept"), set_pending=SAME(AVG_C, OK), set_avg_counters=(OK, AVG_C, "new"),
                set_bearers=(OK, BEAR, None), set_counters=SAME(AVG_C, STATE), set_flows=SAME(AVG_C, INVALID)),
    BEAR: dict(set_avg=(OK, AVG, None), set_pending=SAME(BEAR, STATE), set_avg_counters=SAME(BEAR, STATE),
               set_bearers=(OK, BEAR, None), set_counters=(OK, BEAR_C, "new"), set_flows=SAME(BEAR, INVALID)),
    BEAR_C: dict(set_avg=(OK, AVG, None), set_pending=SAME(BEAR_C, STATE), set_avg_counters=SAME(BEAR_C, STATE),
                 set_bearers=(OK, BEAR_C, "kept"), set_counters=(OK, BEAR_C, "new"), set_flows=SAME(BEAR_C, INVALID)),
}
TABLE_1 = {  # RS_SCHED_PF: averages and flows
    NONE: dict(set_avg=(OK, AVG, None), set_pending=SAME(NONE, STATE), set_avg_counters=SAME(NONE, STATE),
               set_flows=(OK, FLOWS, "new"), set_counters=SAME(NONE, STATE), set_bearers=SAME(NONE, INVALID)),
    AVG: dict(set_avg=(OK, AVG, None), set_pending=SAME(AVG, OK), set_avg_counters=(OK, AVG_C, "new"),
              set_flows=(OK, FLOWS, "new"), set_counters=SAME(AVG, STATE), set_bearers=SAME(AVG, INVALID)),
    AVG_C: dict(set_avg=(OK, AVG_C, "kept"), set_pending=SAME(AVG_C, OK), set_avg_counters=(OK, AVG_C, "new"),
                set_flows=(OK, FLOWS, "new"), set_counters=SAME(AVG_C, STATE), set_bearers=SAME(AVG_C, INVALID)),
    FLOWS: dict(set_avg=(OK, AVG, None), set_pending=SAME(FLOWS, STATE), set_avg_counters=SAME(FLOWS, STATE),
                set_flows=(OK, FLOWS, "new"), set_counters=SAME(FLOWS, STATE), set_bearers=SAME(FLOWS, INVALID)),
}

UES, R, G, CELLS = [2, 2], 4, 2, 2
U = sum(UES)
HAS = np.array([[1, 1], [1, 0], [0, 1], [1, 1]], np.uint8)  # two users lack a bearer: what set_flows masks
AVGS, AVGS2, LAST = np.arange(1, U + 1) * 1000.0, (np.arange(1, 2 * U + 1) * 500.0).reshape(U, 2), 0.1
# the counters a state starts with ("kept") and those the applied setter writes ("new"), per user and per bearer
C1 = {"kept": (np.arange(U) + 11, np.arange(U) + 21), "new": (np.arange(U) + 31, np.arange(U) + 41)}
C2 = {k: (np.stack([a, a + 100], 1), np.stack([b, b + 100], 1)) for k, (a, b) in C1.items()}


def rc_of(rs, fn, *args):
    try:
        fn(*args)
        return OK
    except rs.RadioSaberError as e:
        return e.code


def apply(rs, g, cell, setter, which):
    """one setter on `cell`, with the counters `which` where it takes any; its return code"""
    args = dict(set_avg=(AVGS, LAST), set_pending=(np.arange(U, dtype=np.int32),), set_avg_counters=C1[which],
                set_bearers=(HAS, AVGS2, LAST), set_counters=C2[which], set_flows=(HAS, AVGS2, LAST) + C2[which])[setter]
    return rc_of(rs, getattr(g, setter), cell, *args)


def enter(rs, g, cell, state):
    """`cell` into `state` from whatever state it is in (none: the cell must be fresh), its counters the "kept" ones"""
    other = "set_flows" if g.sched == rs.RS_SCHED_PF else "set_bearers"  # (leaving the averages ends their counters' term)
    path = {NONE: (), AVG: (other, "set_avg"), AVG_C: (other, "set_avg", "set_avg_counters"), BEAR: ("set_avg", "set_bearers"),
            BEAR_C: ("set_avg", "set_bearers", "set_counters"), FLOWS: ("set_flows",)}[state]
    for setter in path:
        assert apply(rs, g, cell, setter, "kept") == OK, f"{setter} on the way to {state}"


def observe(rs, g, cell):
    """the getters that answer, in GETTERS' order; every other one must say RS_ERR_STATE"""
    got = {name: rc_of(rs, getattr(g, name), cell) for name in GETTERS}
    assert set(got.values()) <= {OK, STATE}, got
    return tuple(name for name in GETTERS if got[name] == OK)


def counters_of(g, cell, state):
    if state == AVG_C:
        return g.get_avg_counters(cell)
    return g.get_flows(cell)[3:] if state == FLOWS else g.get_counters(cell)


def expected_counters(state, which):
    if state == AVG_C:
        return C1[which]
    cb, cr = C2[which]
    return (cb * HAS, cr * HAS) if state == FLOWS else (cb, cr)  # (set_flows zeroes a bearer that does not exist, set_counters does not)


def walk(rs, sched, table):
    fresh = []  # cells no setter has touched: two per group

    def fresh_cell():
        if not fresh:
            g = rs.GroupScheduler(rs.SliceConfig(UES), R, G, CELLS, sched=sched)
            fresh.extend([(g, 1), (g, 0)])
        return fresh.pop()

    shared = rs.GroupScheduler(rs.SliceConfig(UES), R, G, CELLS, sched=sched)
    for start, row in table.items():
        for setter, (rc, end, which) in row.items():
            what = f"scheduler {sched}: {setter} from {start}"
            g, cell = fresh_cell() if start == NONE else (shared, 0)
            enter(rs, g, cell, start)
            assert observe(rs, g, cell) == ANSWERS[start], f"{what}: the start state"
            got = apply(rs, g, cell, setter, "new")
            print(f"{what}: returns {got}, then answer {observe(rs, g, cell)}")
            assert got == rc, what
            assert observe(rs, g, cell) == ANSWERS[end], f"{what}: expected {end}"
            if which:
                for a, want in zip(counters_of(g, cell, end), expected_counters(end, which)):
                    np.testing.assert_array_equal(a, want, err_msg=f"{what}: the {which} counters")
            if end == AVG:
                a, pend, last = g.get_avg(cell)
                assert (a == AVGS).all() and last == LAST and (not pend.any() or setter == "set_pending"), what
    assert observe(rs, shared, 1) == (), "a cell no setter named is in no form"


@pytest.mark.gpu
def test_transitions_scheduler_9(rs):
    walk(rs, rs.RS_SCHED_MAXCELL, TABLE_9)


@pytest.mark.gpu
def test_transitions_scheduler_1(rs):
    walk(rs, rs.RS_SCHED_PF, TABLE_1)
