"""The step after the allocation -- the EESM sum over a user's PRBs "in the reference's order", the final CQI, the MCS and the
transport block -- on the directed inputs of tests/link_edges.py: users who hold 1 .. R RBGs of one CQI (where the number and
sequence of the FP64 additions and the one division decide the final CQI: tests/test_link_edge_inputs.py counts, per shape, the
users that four other evaluations would get wrong), means of exactly 0 and subnormal means, a neighbouring or a distant CQI at the
lowest or highest RBG, reports that differ inside an RBG, blocks beyond 110 PRBs, scheduler 1's break `tbs >= data * 8` from both
sides at every reachable (CQI, RBG count) and past every block that shrinks, scheduler 7's wideband CQI in the queue model.  The
aim is the number and sequence of the additions at near-uniform users, not the order of a user's RBGs: no user's final CQI was
found to depend on that (tests/link_edges.py).

Shapes: 25 x 4, 64 x 8 (lanes >= 32, 64-bit lane masks), 32 x 3 (the largest on 32-bit masks in run-time builds), 33 x 2.  Surfaces:
drop-in calls of the built-in kernel and of run-time builds (every case twice), group calls (plain, resident, 4-TTI runs), batches
(built-in and run-time builds, pinned link tables) and one queue-model batch.  Every comparison is bitwise: device == oracle on every
output field, and nprb, final CQI, MCS and TBS == plain_block evaluated on the DEVICE's own map.  For uniform users whose PRB count
is in the recorded list the device's final CQI equals the value the unmodified reference printed (tests/golden/appendix_a.json,
uniform_cqi_roundtrip): device == reference, the first such assertion for this step.

Found by these tests: no difference in the kernels.  That they would find one was tried once, on a scratch build whose P5 sum adds
G * E once per RBG instead of E once per PRB: every test here but the upper-bound scheduler's drop-in calls failed, each within its
first calls on a user of one CQI (user_final_cqi: 25 x 4 at the call of 1, 2, 3, 4, 5, 9 and 1 RBGs, 64 x 8 at the one of 1, 2, 3,
4, 5, 8, 9 and 32)."""
import json

import numpy as np
import pytest

import link_edges as le
import queue_edges
from conftest import GOLDEN
from test_gpu_dropin_oracle import PER_USER, same_call
from test_link_edge_inputs import as_intended, grids, holds, oracle_run, same_as_plain, wide_population

pytestmark = pytest.mark.gpu

KA = json.loads((GOLDEN / "appendix_a.json").read_text())
RECORDED_N = KA["uniform_cqi_roundtrip_n"]


@pytest.fixture(scope="module")
def tabs(rs, oracle):
    """the tables a drop-in or group context uses by default: this host's libm (== the pinned set, tests/test_abi.py)"""
    return le.make_tables(rs.link_tables(), oracle.tables())


@pytest.fixture(scope="module")
def pinned(rs, oracle):
    """a batch's default: the glibc-2.35 set compiled into the library"""
    return le.make_tables(rs.link_tables(pinned=True), oracle.tables())


def report(what, calls, round_trip=None):
    n = le.counts(calls)
    extra = f"; recorded round-trip values met: {round_trip}" if round_trip is not None else ""
    print(f"link edge cases run, {what}: {len(calls)} calls, " + ", ".join(f"{f} {n[f]}" for f in le.FAMILIES if n.get(f)) + extra)
    assert n, what


def calls_of(shape, sched, t):
    """what a scheduler takes on a shape: 1 and 7 every map call, per-RBG and per-PRB, 1 the flows calls as well (every seventh also
    per-PRB), 7 the gate calls; the others the slices calls"""
    if sched == 7:
        return le.map_calls(shape) + le.prb_calls(shape) + le.cached_gate_calls(shape)
    if sched == 1:
        return le.map_calls(shape) + le.prb_calls(shape) + le.cached_flow_calls(shape, t) \
            + [le.prb_variant(c, False) for c in le.cached_flow_calls(shape, t)[::7]]
    return le.cached_slice_calls(shape)


_expected = {}


def expected(oracle, shape, sched, t):
    """[(call, the oracle's outputs)] of one (shape, scheduler), computed once; the oracle has served every case as built"""
    if (shape, sched) not in _expected:
        calls = calls_of(shape, sched, t)
        outs = [oracle_run(oracle, c, sched) for c in calls]
        for c, out in zip(calls, outs):
            as_intended(c, out, t, upper=sched == 10)
        _expected[(shape, sched)] = list(zip(calls, outs))
    return _expected[(shape, sched)]


def config_of(rs, call):
    return rs.SliceConfig([1] * call.n, weight=list(call.w)) if call.kind == "slices" else rs.SliceConfig([call.n])


def call_kw(call):
    cqi, prb, avg = grids(call)
    kw = dict(cqi=None if call.per_prb else cqi, avg_rate=avg)
    if call.per_prb:
        kw["cqi_prb"] = prb
    if call.kind in ("flows", "gate"):
        kw["data_to_transmit" if call.kind == "flows" else "required_rbs"] = np.array(call.data, np.int32)
    return kw


def round_trip(call, res, upper=False):
    """device == reference: every user whose PRBs all report one CQI and whose PRB count the reference's round trip recorded;
    returns how many"""
    n = 0
    for i, rbgs in enumerate(holds(call, res, upper)):
        if len(rbgs) * call.G in RECORDED_N:
            prbs = le.plain_prbs(call.G, rbgs, call.rows()[i], call.per_prb)
            if len(set(prbs)) == 1:
                want = KA["uniform_cqi_roundtrip"][str(prbs[0])][RECORDED_N.index(len(prbs))]
                assert int(res.user_nprb[i]) == len(prbs) and int(res.user_final_cqi[i]) == want, \
                    f"{call.name} user {i}: CQI {prbs[0]} x {len(prbs)} PRBs, the reference printed {want}"
                n += 1
    return n


def check(res, out, call, sched, t, what):
    same_call(res, out, None, f"{what} {call.name}", upper=sched == 10)
    same_as_plain(call, res, t, what, upper=sched == 10)
    return round_trip(call, res, upper=sched == 10)


# ---------------------------------------------------------------------------------------------------------------------------
# drop-in calls
# ---------------------------------------------------------------------------------------------------------------------------

def _dropin(rs, oracle, sched, shape, t, jit):
    R, G = le.SHAPES[shape]
    exp = expected(oracle, shape, sched, t)
    what = f"sched {sched} {shape} {'run-time build' if jit else 'built-in'}"
    ts = rs.TtiScheduler(config_of(rs, exp[0][0]), R, G, sched=sched, jit=jit)
    met = 0
    for rnd in range(2 if jit else 1):      # (a run-time build's first calls run beside the built-in kernel)
        for call, out in exp:
            if call.kind == "slices":
                ts.slice_offset = call.offset
            met += check(ts.schedule_tti(**call_kw(call)), out, call, sched, t, what)
    if jit:
        assert ts.jit_status()[0] == 1, ts.jit_status()
    ts.close()
    if shape in ("A", "B"):
        assert met > 0, f"{what}: no recorded round-trip value met"
    report(what, [c for c, _ in exp], met)


BUILT_IN = [(s, sh) for s in (1, 7) for sh in le.SHAPES] + [(s, sh) for s in (9, 8) for sh in ("A", "B")] + [(s, "A") for s in (10, 101, 103)]


@pytest.mark.parametrize("sched,shape", BUILT_IN, ids=[f"{s}-{sh}" for s, sh in BUILT_IN])
def test_dropin_calls(rs, oracle, tabs, sched, shape):
    """Schedulers 1 and 7: uniform, zero, mixed, per-PRB, (1) flow_break / shrinking_block and (7) the required_rbs gate, on all four
    shapes; the transport schedulers: one user per slice, quotas 1, 2, 3, 4, 5, 8, 9, R (64 x 8: 16, 32, 33, 64 as well) at every CQI"""
    _dropin(rs, oracle, sched, shape, tabs, False)


RUNTIME = [(1, "A"), (7, "A"), (9, "A"), (1, "C"), (7, "C"), (9, "C"), (9, "D"), (9, "B")]


@pytest.mark.parametrize("sched,shape", RUNTIME, ids=[f"{s}-{sh}" for s, sh in RUNTIME])
def test_dropin_runtime_builds(rs, oracle, tabs, sched, shape):
    """The context's own build, every case twice: 32-bit lane masks on 25 x 4 and 32 x 3, 64-bit ones on 33 x 2 and 64 x 8"""
    _dropin(rs, oracle, sched, shape, tabs, True)


# ---------------------------------------------------------------------------------------------------------------------------
# group calls
# ---------------------------------------------------------------------------------------------------------------------------

GROUP_CELLS = 15


@pytest.mark.parametrize("sched", [9, 1])
def test_group_calls_plain_and_resident(rs, oracle, tabs, sched):
    """25 x 4, 15 cells a launch, one case call per cell: a plain launch; the resident launch at now == last_update (the averages
    are used as set).  Scheduler 1: the per-RBG map calls in both forms, the flows calls (data_to_transmit) in plain launches."""
    R, G = le.SHAPES["A"]
    exp = [(c, o) for c, o in expected(oracle, "A", sched, tabs) if not c.per_prb]
    g = rs.GroupScheduler(config_of(rs, exp[0][0]), R, G, GROUP_CELLS, sched=sched)
    met = 0
    chunks = []      # (the cells of a launch give the same optional inputs: map calls and flows calls go in launches of their own)
    for kind in ("slices", "map", "flows"):
        mine = [x for x in exp if x[0].kind == kind]
        for at in range(0, len(mine), GROUP_CELLS):
            chunk = mine[at:at + GROUP_CELLS]
            chunks.append(chunk + mine[:GROUP_CELLS - len(chunk)])
    for chunk in chunks:
        for form in ("plain", "resident"):
            if form == "resident" and chunk[0][0].kind == "flows":
                continue
            calls = [call_kw(c) for c, _ in chunk]
            for k, (c, _) in enumerate(chunk):
                if c.kind == "slices":
                    g.set_slice_offset(k, c.offset)
                if form == "resident":
                    g.set_avg(k, calls[k].pop("avg_rate"), 0.1)
            res = g.schedule_tti(calls) if form == "plain" else g.schedule_tti_at(calls, 0.1)
            for k, (c, out) in enumerate(chunk):
                met += check(res[k], out, c, sched, tabs, f"group sched {sched} {form} cell {k}")
    g.close()
    assert met > 0
    report(f"group sched {sched} plain and resident", [c for c, _ in exp], met)


RUN_TTIS = 4


def test_group_runs_on_constant_reports(rs, oracle, tabs):
    """Scheduler 9, 25 x 4: run_at over 4 TTIs in one launch on the slices calls' constant reports.  The first TTI serves the cases;
    afterwards the offsets and the averages move, the uniform users recur with other RBG counts; user_* of every TTI is checked"""
    R, G = le.SHAPES["A"]
    calls = le.cached_slice_calls("A")
    ticks = oracle.clock_ticks(100, RUN_TTIS)
    rng = np.random.default_rng(77)
    g = rs.GroupScheduler(config_of(rs, calls[0]), R, G, GROUP_CELLS, sched=9)
    met, counts = 0, set()
    for at in range(0, len(calls), GROUP_CELLS):
        chunk = calls[at:at + GROUP_CELLS]
        assert len(chunk) == GROUP_CELLS
        rands = rng.integers(0, 2**31 - 64, (GROUP_CELLS, RUN_TTIS, 2)).astype(np.int32)
        cells = []
        for k, c in enumerate(chunk):
            cqi, _, avg = grids(c)
            cell = oracle.Cell([1] * c.n, R, G, 9, weights=c.w)
            cell.set_slice_offset(c.offset)
            cell.set_cqi(cqi)
            cell.set_avg_rate(avg)
            cell.set_last_update(0.1)
            cells.append(cell)
            g.set_slice_offset(k, c.offset)
            g.set_avg(k, avg, 0.1)
        res = g.run_at([dict(cqi=grids(c)[0], cqi_epoch=1 + at) for c in chunk], ticks, rands)
        for k, c in enumerate(chunk):
            for n in range(RUN_TTIS):
                out = cells[k].new_out()
                assert cells[k].step(float(ticks[n]), int(rands[k, n, 0]), int(rands[k, n, 1]), out) == 0
                if n == 0:
                    as_intended(c, out, tabs)
                met += check(res[k][n], out, c, 9, tabs, f"run sched 9 cell {k} TTI {n}")
                counts |= {(n, int(x)) for x in res[k][n].user_nprb}
            assert g.slice_offset(k).tobytes() == cells[k].state()["slice_state"].tobytes(), f"run sched 9 {c.name}: offsets afterwards"
    g.close()
    assert len({x for n, x in counts if n > 0} - {x for n, x in counts if n == 0}) > 0, "the later TTIs repeat the first one's RBG counts"
    report("group runs sched 9", calls, met)


# ---------------------------------------------------------------------------------------------------------------------------
# batches
# ---------------------------------------------------------------------------------------------------------------------------

BATCH_TTIS = (1, 2)
SEED0 = 5200


class _Row:
    """one TTI of one cell of a logged batch, with the field names of a call's result"""

    def __init__(self, log, k, j):
        self.rbg_to_user = log["rbg_to_user"][k, j].astype(np.int32)
        self.user_nprb, self.user_final_cqi = log["nprb"][k, j], log["final_cqi"][k, j]
        self.user_mcs, self.user_tbs_bits = log["mcs"][k, j], log["tbs_bits"][k, j]


def _batch(rs, oracle, sched, calls, jit, t):
    """One batch, cell k started from call k: averages (and offsets) through write_state, two identical CQI epochs, 1 + 2 logged
    TTIs on the batch's own rand() streams; nprb, final CQI, MCS and TBS of every TTI against the stepped oracle and against the
    plain model on the batch's own maps"""
    K, c0 = len(calls), calls[0]
    R, G = c0.R, c0.G
    seeds = np.arange(K, dtype=np.uint32) + SEED0
    b = rs.BatchScheduler(config_of(rs, c0), R, G, K, sched=sched, jit=jit, cqi_epoch_wrap=True)
    b.seed(seeds)
    b.upload_cqi_epochs(np.stack([np.stack([grids(c)[0]] * 2) for c in calls]))
    state = dict(avg_rate=np.stack([grids(c)[2] for c in calls]))
    if c0.kind == "slices":
        state["slice_state"] = np.array([c.offset for c in calls])
    b.write_state(**state)
    logs = [b.run_logged(n) for n in BATCH_TTIS]
    status = b.jit_status()
    b.close()
    assert status[0] == (1 if jit else 0), status
    ticks = oracle.clock_ticks(100, sum(BATCH_TTIS))
    met = 0
    for k, c in enumerate(calls):
        cqi, _, avg = grids(c)
        cell = oracle.Cell([1] * c.n, R, G, sched, weights=c.w) if c.kind == "slices" else oracle.Cell([c.n], R, G, sched)
        if c.kind == "slices":
            cell.set_slice_offset(c.offset)
        cell.set_cqi(cqi)
        cell.set_avg_rate(avg)
        cell.set_last_update(0.1)
        rng = oracle.Rng(int(seeds[k]))
        n = 0
        for log, ttis in zip(logs, BATCH_TTIS):
            for j in range(ttis):
                what = f"batch sched {sched} {'run-time build' if jit else 'built-in'} {c.name} TTI {n}"
                r0, r1 = (rng.rand(), rng.rand()) if sched != 7 else (0, 0)
                out = cell.new_out()
                assert cell.step(float(ticks[n]), r0, r1, out) == 0
                if n == 0:
                    as_intended(c, out, t)
                row = _Row(log, k, j)
                np.testing.assert_array_equal(row.rbg_to_user, out.rbg_to_user, err_msg=f"{what}: RBG map")
                for f in PER_USER:
                    np.testing.assert_array_equal(getattr(row, f), getattr(out, f), err_msg=f"{what}: {f}")
                same_as_plain(c, row, t, what)
                met += round_trip(c, row)
                n += 1
    return met


BATCHES = [(9, "A", False), (9, "A", True), (8, "A", False), (8, "A", True), (7, "A", False), (7, "A", True), (9, "B", False), (9, "B", True)]


@pytest.mark.parametrize("sched,shape,jit", BATCHES, ids=[f"{s}-{sh}-{'jit' if j else 'builtin'}" for s, sh, j in BATCHES])
def test_batches(rs, oracle, pinned, sched, shape, jit):
    """Schedulers 9 and 8: the slices calls, one per cell; scheduler 7: the per-RBG map calls (one slice of 8 users).  The run-time
    builds of scheduler 9 are the held-winner kernels the benchmark measures"""
    calls = le.map_calls(shape) if sched == 7 else le.cached_slice_calls(shape)
    met = _batch(rs, oracle, sched, calls, jit, pinned)
    assert met > 0
    report(f"batch sched {sched} {shape} {'run-time build' if jit else 'built-in'}", calls, met)


def test_lean_build_of_the_benchmark_scheduler(rs, oracle, pinned, monkeypatch):
    """Scheduler 9 on 64 x 8, one unlogged launch of the lean run-time build: the counters it leaves are the stepped oracle's, whose
    blocks equal the plain model's (tests/test_link_edge_inputs.py)"""
    monkeypatch.setenv("RS_JIT_LEAN_MIN_TTIS", "1")
    calls = le.cached_slice_calls("B")
    K, (R, G), T = len(calls), le.SHAPES["B"], 3
    seeds = np.arange(K, dtype=np.uint32) + SEED0
    b = rs.BatchScheduler(config_of(rs, calls[0]), R, G, K, sched=9, jit=True, cqi_epoch_wrap=True)
    b.seed(seeds)
    b.upload_cqi_epochs(np.stack([np.stack([grids(c)[0]] * 2) for c in calls]))
    b.write_state(avg_rate=np.stack([grids(c)[2] for c in calls]), slice_state=np.array([c.offset for c in calls]))
    b.run(T)
    st, status = b.state(), b.jit_status()
    b.close()
    assert status[0] == 1 and "unavailable" not in status[1], status
    ticks = oracle.clock_ticks(100, T)
    for k, c in enumerate(calls):
        cell = oracle.Cell([1] * c.n, R, G, 9, weights=c.w)
        cell.set_slice_offset(c.offset)
        cell.set_cqi(grids(c)[0])
        cell.set_avg_rate(grids(c)[2])
        cell.set_last_update(0.1)
        rng = oracle.Rng(int(seeds[k]))
        for n in range(T):
            out = cell.new_out()
            assert cell.step(float(ticks[n]), rng.rand(), rng.rand(), out) == 0
            same_as_plain(c, out, pinned, f"oracle TTI {n}")
        want = cell.state()
        for f in ("cum_bytes", "cum_rbs"):
            np.testing.assert_array_equal(st[f][k], want[f], err_msg=f"lean build {c.name}: {f}")
        assert st["avg_rate"][k].tobytes() == want["avg_rate"].tobytes() and st["slice_state"][k].tobytes() == want["slice_state"].tobytes(), c.name
    report("lean build sched 9 B", calls)


@pytest.mark.parametrize("shape", ["A", "B"])
@pytest.mark.parametrize("jit", [False, True], ids=["builtin", "jit"])
def test_wideband_cqi_in_the_queue_model(rs, oracle, pinned, shape, jit):
    """Scheduler 7 with finite queues (rs_phase_p3.inc: the wideband CQI over all R * G PRBs sets m_requiredRBs): rows of one CQI whose
    wideband CQI is another, data for which that changes the number of RBGs.  The RBG count of user 0 in the first TTI equals the
    plain model's; maps, blocks and the bearers' state afterwards equal the stepped oracle's"""
    from test_gpu_queue_edges import _batch as queue_batch, _check_final
    R, G = le.SHAPES[shape]
    p = wide_population(oracle, pinned, shape)
    run = queue_edges.oracle_run(oracle, p)
    done = {}
    for c in range(p.n_cells):
        for u, m in enumerate(queue_edges.plain_cell(oracle, p, run, c)):
            for k, tti in m["done"].items():
                done[(c, u, k)] = tti
    b = queue_batch(rs, p, jit=jit)
    log = b.run_logged(p.n_ttis, bearers=True)
    what = f"wide {shape} {'run-time build' if jit else 'built-in'}"
    for c, x in enumerate(p.plan):
        assert log["nprb"][c, 0, 0] == x["rbgs"] * G != x["rbgs_if_c"] * G, f"{what} cell {c} {x}: {log['nprb'][c, 0, 0]} PRBs"
        for n in range(p.n_ttis):
            held = le.holdings(2, log["rbg_to_user"][c, n])
            want = le.plain_blocks(pinned, G, held, [[x["c"]] * R] * 2)
            have = [[int(log[f][c, n, u]) for f in ("nprb", "final_cqi", "mcs", "tbs_bits")] for u in range(2)]
            assert have == want, f"{what} cell {c} TTI {n}: blocks against the plain model on the batch's own map"
    np.testing.assert_array_equal(log["rbg_to_user"], run["maps"], err_msg=f"{what}: RBG map")
    for f, g in (("tbs_bits", "tbs"), ("nprb", "nprb"), ("final_cqi", "final_cqi"), ("bearer_bytes", "bearer_bytes")):
        np.testing.assert_array_equal(log[f], run[g], err_msg=f"{what}: {f}")
    _check_final(rs, p, run, done, b, what)
    b.close()
    print(f"link edge cases run, {what}: {p.n_cells} cells of the wide family")
