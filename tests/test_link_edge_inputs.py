"""The directed inputs of tests/link_edges.py on the CPU: the plain model (one addition per PRB, one division, the reference's dB
expression; the transport block with the rule beyond 110 PRBs) equals the oracle's rso_final_cqi and rso_tbs_bits on every case and
the values the unmodified reference printed for uniform users (tests/golden/appendix_a.json, uniform_cqi_roundtrip); the cases bind
-- on every shape with G >= 2 each of four other evaluations of the mean gives some uniform users another final CQI, the `zero`
family holds subnormal means, the blocks beyond 110 PRBs hold all three branches of the rule, every reachable (c, k) of scheduler
1's break is met from both sides and every unreachable one walked past --; and the oracle, run on the constructed calls, hands every
user exactly the RBGs the case wants and derives nprb, final CQI, MCS and TBS as plain_block does from the oracle's own map.

Found by these tests: no difference between the oracle, the plain model and the recorded values."""
import json

import numpy as np
import pytest

import link_edges as le
from conftest import GOLDEN
from test_gpu_dropin_oracle import PER_USER, oracle_call

KA = json.loads((GOLDEN / "appendix_a.json").read_text())
UNREACHABLE = {"A": 6, "B": 111, "C": 9}      # of 375, 960 and 480 (c, k): measured with the oracle when the families were designed


@pytest.fixture(scope="module")
def tabs(rs, oracle):
    return le.make_tables(rs.link_tables(), oracle.tables())


def grids(call):
    """(cqi [n][R], cqi_prb [n][R * G] or None, avg [n]) as arrays"""
    prb = np.array(call.cqi_prb, np.uint8) if call.per_prb else None
    return np.array(call.cqi, np.uint8), prb, np.array(call.avg, np.float64)


_cells = {}


def oracle_run(oracle, call, sched):
    """the oracle's answer to one call (a fresh cell per slices call: the offsets are part of the case)"""
    cqi, prb, avg = grids(call)
    if call.kind == "slices":
        cell = oracle.Cell([1] * call.n, call.R, call.G, sched, weights=call.w)
        cell.set_slice_offset(call.offset)
        return oracle_call(cell, None, cqi, avg)
    key = (sched, call.shape, call.n)
    if key not in _cells:
        _cells[key] = oracle.Cell([call.n], call.R, call.G, sched)
    gate = np.array(call.data, np.int32) if call.kind in ("flows", "gate") else None
    return oracle_call(_cells[key], None, cqi, avg, slice_id=0 if sched == 7 else -1, gate=gate, cqi_prb=prb)


def holds(call, got, upper=False):
    """what every user of the call holds, as sorted RBG lists: from the map, for the upper-bound scheduler (10) from its lists"""
    return le.holdings(call.n, got.rbg_to_user, got.upper_rbg if upper else None)


def as_intended(call, got, t, upper=False):
    """the number of cases of the call, after asserting that each holds what it was built to hold"""
    held = holds(call, got, upper)
    n = 0
    for i, u in enumerate(call.users):
        if call.kind == "map":
            assert held[i] == sorted(u.held), f"{call.name}: user {i} ({u.family} {u.tag}) holds {held[i]}"
        elif call.kind == "slices":
            assert len(held[i]) == u.k, f"{call.name}: slice {i} holds {len(held[i])} RBGs"
        elif call.kind == "gate":
            at = sum(v.k for v in call.users[:i])
            assert held[i] == list(range(at, at + u.k)), f"{call.name}: user {i} holds {held[i]}"
        elif u.family != "idle":
            assert len(held[i]) == u.takes and held[i] == list(range(held[i][0], held[i][0] + u.takes)), f"{call.name}: flow {i}"
            if u.side == "stops":
                assert u.takes == u.k and le.uniform_tbs(t, call.G, u.c, u.k) >= u.data * 8, f"{call.name}: flow {i}"
            else:
                assert u.takes > u.k or u.k == call.R, f"{call.name}: flow {i} stopped at {u.takes} RBGs"
                assert le.uniform_tbs(t, call.G, u.c, u.k) < u.data * 8, f"{call.name}: flow {i}"
        n += u.family not in ("idle", "filler")
    return n


def same_as_plain(call, got, t, what, upper=False):
    """nprb, final CQI, MCS and TBS of every user against plain_block on the map that came with them"""
    want = le.plain_blocks(t, call.G, holds(call, got, upper), call.rows(), call.per_prb)
    have = [[int(getattr(got, f)[i]) for f in PER_USER] for i in range(call.n)]
    assert have == want, f"{what} {call.name}: (nprb, final CQI, MCS, TBS) against the plain model on its own map"


def all_calls(shape, t):
    return le.map_calls(shape) + le.prb_calls(shape) + le.cached_flow_calls(shape, t) + le.cached_gate_calls(shape) + le.cached_slice_calls(shape)


# ---------------------------------------------------------------------------------------------------------------------------
# the plain model against the oracle's two functions and the recorded values
# ---------------------------------------------------------------------------------------------------------------------------

def test_plain_final_cqi_equals_the_oracle_on_every_case(oracle, tabs):
    seen = set()
    for shape in le.SHAPES:
        for call in all_calls(shape, tabs):
            for i, u in enumerate(call.users):
                rbgs = list(u.held) if call.kind == "map" else list(range(u.takes if call.kind == "flows" else u.k))
                if u.family == "idle":
                    continue
                prbs = tuple(le.plain_prbs(call.G, rbgs, call.rows()[i], call.per_prb))
                if prbs and prbs not in seen:
                    seen.add(prbs)
                    assert le.plain_final_cqi(tabs.E, tabs.sinr, prbs) == oracle.final_cqi(np.array(prbs, np.uint8)), f"{call.name} user {i}"
    print(f"link edge cases: {len(seen)} different PRB lists")
    assert len(seen) > 4000


def test_plain_final_cqi_equals_the_recorded_round_trip(tabs):
    for c, want in KA["uniform_cqi_roundtrip"].items():
        got = [le.plain_final_cqi(tabs.E, tabs.sinr, [int(c)] * n) for n in KA["uniform_cqi_roundtrip_n"]]
        assert got == want, f"CQI {c}"


def test_plain_tbs_equals_the_oracle(oracle, tabs):
    used = set()
    for shape, (R, G) in le.SHAPES.items():
        for call in le.map_calls(shape) + le.prb_calls(shape):
            for i, u in enumerate(call.users):
                if u.held:
                    used.add(le.plain_block(tabs, G, list(u.held), call.rows()[i], call.per_prb)[:2])
        for c in range(1, 16):
            for k in range(1, R + 1):
                used.add((k * G, le.plain_final_cqi(tabs.E, tabs.sinr, [c] * (k * G))))
    for nprb, fc in used:
        assert le.plain_tbs_bits(tabs, fc, nprb) == oracle.lib().rso_tbs_bits(tabs.cqi_to_mcs[fc - 1], nprb), (fc, nprb)
    assert le.plain_tbs_bits(tabs, 15, 120) == KA["tbs_120prb_cqi15_bits"]
    print(f"link edge cases: {len(used)} different (PRB count, final CQI)")


# ---------------------------------------------------------------------------------------------------------------------------
# the cases bind
# ---------------------------------------------------------------------------------------------------------------------------

def test_uniform_users_separate_the_evaluations(tabs):
    for shape, (R, G) in le.SHAPES.items():
        users = {(u.c, u.k) for call in le.uniform_calls(shape) for u in call.users if u.family == "uniform"}
        assert users == {(c, k) for c in range(1, 16) for k in range(1, R + 1)}, f"{shape}: not every (c, k)"
        differ = {}
        for c, k in users:
            ref = le.plain_final_cqi(tabs.E, tabs.sinr, [c] * (k * G))
            for name, fc in le.alternatives(tabs, G, c, k).items():
                differ[name] = differ.get(name, 0) + int(fc != ref)
        print(f"uniform users of {shape} ({R} x {G}, {len(users)}) whose final CQI another evaluation changes: "
              + ", ".join(f"{name} {n}" for name, n in differ.items()))
        assert all(n > 0 for n in differ.values()), f"{shape}: {differ}"


def test_layouts_straddle_the_lane_halves():
    for shape in ("B", "D"):
        n = 0
        for call in le.uniform_calls(shape):
            for u in call.users:
                rb = sorted(u.held)
                if u.family == "uniform" and rb and rb[0] <= 31 < rb[-1] and rb != list(range(rb[0], rb[-1] + 1)):
                    n += 1
        print(f"uniform users of {shape} whose RBGs are not contiguous and lie on both sides of lanes 31/32: {n}")
        assert n >= 50
    first = le.uniform_calls("A")[0]
    assert sorted(u.k for u in first.users if u.family == "uniform") == [1, 1, 2, 3, 4, 5, 9]


def test_zero_family_holds_exact_zeros_and_subnormal_means(tabs):
    assert tabs.E[15] == 0.0 and 0 < tabs.E[14] < 2e-307
    for shape, (R, G) in le.SHAPES.items():
        zero = sub = flushed = 0
        for call in le.zero_calls(shape) + le.single_prb_calls(shape):
            for i, u in enumerate(call.users):
                if u.family not in ("zero", "prb"):
                    continue
                prbs = le.plain_prbs(G, list(u.held), call.rows()[i], call.per_prb)
                x = le.plain_mean(tabs.E, prbs)
                zero += int(x == 0)
                if 0 < x < le.MIN_NORMAL:
                    sub += 1
                    # flushed to zero the mean would say 15
                    assert le.cqi_from_mean(tabs.sinr, x) == 14 != le.cqi_from_mean(tabs.sinr, 0.0), call.name
                    flushed += 1
        print(f"zero family of {shape}: {zero} users with a mean of exactly 0, {sub} with a subnormal mean")
        assert zero >= 10 and sub >= 10 and flushed == sub


def test_mixed_family_has_both_positions(tabs):
    for shape in le.SHAPES:
        tags = {(u.tag.split("(")[1]) for call in le.mixed_calls(shape) for u in call.users if u.family == "mixed"}
        assert tags == {"neighbour, lowest)", "neighbour, highest)", "distant, lowest)", "distant, highest)"}
        cs = {u.c for call in le.mixed_calls(shape) for u in call.users if u.family == "mixed"}
        assert cs == set(range(1, 16))


def test_blocks_beyond_110_prbs_hold_every_branch(tabs):
    R, G = le.SHAPES["B"]
    seen = {}
    for call in le.map_calls("B") + le.prb_calls("B"):
        for i, u in enumerate(call.users):
            nprb, fc = le.plain_block(tabs, G, list(u.held), call.rows()[i], call.per_prb)[:2]
            if nprb > 110 and u.family not in ("idle", "filler"):
                itbs = tabs.mcs_to_itbs[tabs.cqi_to_mcs[fc - 1]]
                kind = "n % 5 != 0" if nprb % 5 else ("n % 5 == 0, iTBS <= 23" if itbs <= 23 else "n % 5 == 0, iTBS > 23")
                seen[kind] = seen.get(kind, 0) + 1
                if kind == "n % 5 == 0, iTBS > 23":
                    assert fc in (14, 15)
    print("tbs family (B, more than 110 PRBs): " + ", ".join(f"{k}: {n}" for k, n in sorted(seen.items())))
    assert set(seen) == {"n % 5 != 0", "n % 5 == 0, iTBS <= 23", "n % 5 == 0, iTBS > 23"} and min(seen.values()) >= 10


def test_flow_break_meets_every_reachable_block_from_both_sides(tabs):
    for shape, (R, G) in le.SHAPES.items():
        bad = le.unreachable(tabs, R, G)
        if shape in UNREACHABLE:
            assert len(bad) == UNREACHABLE[shape], f"{shape}: {len(bad)} unreachable (c, k)"
        sides, past = {}, set()
        for call in le.cached_flow_calls(shape, tabs):
            assert sum(u.takes for u in call.users) <= R and call.n == le.MAP_USERS
            for u in call.users:
                if u.family == "idle":
                    continue
                if u.family == "flow_break":
                    sides.setdefault((u.c, u.k), set()).add(u.side)
                else:
                    assert u.family == "shrinking_block" and (u.takes > u.k or u.k == R)
                    past.add((u.c, u.k))
        every = {(c, k) for c in range(1, 16) for k in range(1, R + 1)}
        assert set(sides) == every - bad and all(s == {"stops", "goes on"} for s in sides.values()) and past == bad
        shrinks = sum(1 for c, k in bad if le.uniform_tbs(tabs, G, c, k) < le.uniform_tbs(tabs, G, c, k - 1))
        print(f"flow_break {shape}: {len(sides)} of {len(every)} (c, k) met from both sides, {len(bad)} unreachable "
              f"({shrinks} where the block shrinks), {len(le.cached_flow_calls(shape, tabs))} calls")
        assert len(sides) == len(every) - len(bad)


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle on the constructed calls
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", list(le.SHAPES))
@pytest.mark.parametrize("sched", [7, 1])
def test_oracle_serves_the_maps_and_equals_the_plain_model(oracle, tabs, sched, shape):
    R, G = le.SHAPES[shape]
    reached, gated = set(), set()
    calls = le.map_calls(shape) + le.prb_calls(shape) + (le.cached_gate_calls(shape) if sched == 7 else [])
    for call in calls:
        out = oracle_run(oracle, call, sched)
        as_intended(call, out, tabs)
        same_as_plain(call, out, tabs, f"oracle sched {sched}")
        if call.kind == "gate":
            gated |= {(u.c, u.k) for u in call.users if u.family == "uniform"}
        elif not call.per_prb:
            reached |= {(u.c, u.k) for u in call.users if u.family == "uniform"}
    every = {(c, k) for c in range(1, 16) for k in range(1, R + 1)}
    assert reached == every and (sched != 7 or gated == every), f"sched {sched} {shape}: uniform coverage"
    n = le.counts(calls)
    print(f"oracle sched {sched} {shape}: " + ", ".join(f"{f} {k}" for f, k in n.items()))


@pytest.mark.parametrize("shape", list(le.SHAPES))
def test_oracle_flows_stop_where_the_plain_model_stops(oracle, tabs, shape):
    R, G = le.SHAPES[shape]
    stops = set()
    for call in le.cached_flow_calls(shape, tabs):
        out = oracle_run(oracle, call, 1)
        assert out.rbg_to_user.tolist() == le.plain_flows(tabs, R, G, call.cqi, call.avg, call.data), f"{call.name}: RBG map"
        as_intended(call, out, tabs)
        same_as_plain(call, out, tabs, "oracle sched 1")
        stops |= {(u.c, u.k) for u in call.users if u.side == "stops"}
    assert len(stops) == 15 * R - len(le.unreachable(tabs, R, G))


@pytest.mark.parametrize("shape", list(le.SHAPES))
@pytest.mark.parametrize("sched", le.TRANSPORT)
def test_oracle_quotas_hand_every_slice_its_count(oracle, tabs, sched, shape):
    reached = set()
    for call in le.cached_slice_calls(shape):
        out = oracle_run(oracle, call, sched)
        assert out.quota_rbgs.tolist() == [u.k for u in call.users], call.name
        as_intended(call, out, tabs, upper=sched == 10)
        same_as_plain(call, out, tabs, f"oracle sched {sched}", upper=sched == 10)
        reached |= {(u.c, u.k) for u in call.users}
    assert reached >= {(c, k) for c in range(1, 16) for k in le.TRANSPORT_K[shape]}, f"sched {sched} {shape}"


# ---------------------------------------------------------------------------------------------------------------------------
# scheduler 7's wideband CQI in the queue model
# ---------------------------------------------------------------------------------------------------------------------------

def wide_population(oracle, t, shape):
    return le.wide_population(t, shape, float(oracle.clock_ticks(100, 1)[0]))


@pytest.mark.parametrize("shape", ["A", "B"])
def test_wide_family_changes_the_rbg_count(oracle, tabs, shape):
    """the wideband CQI of a uniform row differs from the row's CQI, m_requiredRBs allows another number of RBGs than it would with
    the row's CQI, and the stepped oracle hands user 0 exactly that many in the first TTI; the per-packet model of
    tests/queue_edges.py agrees with the oracle on the whole run"""
    import queue_edges
    R, G = le.SHAPES[shape]
    p = wide_population(oracle, tabs, shape)
    assert p.n_cells >= 3 and all(x["wide"] != x["c"] and x["rbgs"] != x["rbgs_if_c"] for x in p.plan)
    run = queue_edges.oracle_run(oracle, p)
    for c, x in enumerate(p.plan):
        assert oracle.final_cqi(np.full(R * G, x["c"], np.uint8)) == x["wide"], x
        assert run["nprb"][c, 0, 0] == x["rbgs"] * G, f"wide {shape} cell {c} {x}: user 0 holds {run['nprb'][c, 0, 0]} PRBs"
        held = le.holdings(2, run["maps"][c, 0])
        want = le.plain_blocks(tabs, G, held, [[x["c"]] * R] * 2)
        have = [[int(run[k][c, 0, u]) for k in ("nprb", "final_cqi")] + [int(run["tbs"][c, 0, u])] for u in range(2)]
        assert have == [[w[0], w[1], w[3]] for w in want], f"wide {shape} cell {c}: blocks against the plain model"
    bad, _ = queue_edges.disagreements(oracle, p, run)
    assert not bad, bad
    print(f"wide {shape}: {p.n_cells} cells, CQIs {sorted({x['c'] for x in p.plan})}, "
          f"RBG counts (wideband, row's CQI) {sorted({(x['rbgs'], x['rbgs_if_c']) for x in p.plan})}")
