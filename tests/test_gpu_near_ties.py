"""The two-stage arg-max on the inputs that can break it: users whose exact FP64 metrics differ by nothing, by one ulp of
a double, by 2^-45 ... 2^-18 relative -- in the same block of 8, 16 or 32 users, in neighbouring blocks, two blocks apart, at a slice's
first and last user, either side of scheduler 1's segment boundaries and of scheduler 7's run boundaries, in one and in two CQI classes,
several at once (tests/near_ties.py).  tests/test_near_tie_inputs.py proves on the CPU that these inputs bind and that the oracle's scans
agree with a plain numpy scan on them; here the kernels meet them: drop-in calls (built-in and run-time builds, per-RBG and per-PRB
reports, subset calls, the exact-scan fall-back), group calls (plain, resident and scheduler 1's flows form, 45 TTIs on the device's own
EWMA) and batches (speculation, scheduler 7's split runs, 90 TTIs in three launches; held winners on the populations placed around the
hold margin mu).  Every comparison is bitwise: device == oracle == plain numpy.

Scheduler 7's run boundaries exist in the batches only: drop-in and group contexts scan the served slice unsplit."""
import numpy as np
import pytest

import near_ties as nt
from test_gpu_dropin_oracle import oracle_call, same_call
from test_gpu_group_resident import _same_by_id
from test_group_flows_abi import INFINITE, LAST0
from test_near_tie_inputs import subset_ids

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eff(oracle):
    return np.array([0.0] + [oracle.lib().rso_efficiency_from_cqi(c) for c in range(1, 16)])


def rbg_size(R):
    return 2 if R == 4 else 4


def pops_of(eff, sched):
    if sched == 1:
        return nt.pf_set(eff)
    if sched == 7:
        return nt.nvs_set(eff)   # (drop-in and group contexts scan the served slice unsplit)
    return nt.transport_set(eff, sched)


def one_call(oracle, cell, p, ids=None, per_prb=False):
    """(keyword arguments of schedule_tti, the ids same_call wants, the oracle's answer) of one call on population p; scheduler 7
    passes the served slice 1 alone."""
    G = cell.rbg_size
    if p.sched == 7:
        ids = np.arange(int(p.first[1]), int(p.first[2]), dtype=np.int32)
    rows = slice(None) if ids is None else ids
    cqi, avg = p.cqi[rows], p.avg[rows]
    kw = dict(cqi=cqi, avg_rate=avg, rand0=5, rand1=9)
    okw = dict(rand0=5, rand1=9)
    if ids is not None:
        kw["user_id"] = ids
    if p.sched == 7:
        okw["slice_id"] = 1
    if per_prb:
        prb = np.repeat(cqi, G, axis=1)
        kw.update(cqi=None, cqi_prb=prb)
        okw["cqi_prb"] = prb
    out = oracle_call(cell, ids, cqi, avg, **okw)
    return kw, ids, out


def check_plain(p, eff, out, ids=None):
    """the oracle's answer against the plain numpy scan, where one call's outputs determine the winners"""
    want = nt.winners(p, eff, ids)
    if p.sched == 1:
        np.testing.assert_array_equal(out.rbg_to_user, want[0], err_msg=p.name)
    elif p.sched == 7:
        np.testing.assert_array_equal(out.rbg_to_user, want[1], err_msg=p.name)
    else:
        np.testing.assert_array_equal(out.slice_user.T, want, err_msg=p.name)


@pytest.mark.parametrize("sched", [1, 7, 8, 9, 10])
def test_dropin_calls(rs, oracle, eff, sched):
    """Every population of the scheduler's set through the built-in kernel: the full call, and for the transport schedulers a call
    without three users in front of slice 1's pairs (the pairs land in other block positions)."""
    for p in pops_of(eff, sched):
        G = rbg_size(p.R)
        ts = rs.TtiScheduler(rs.SliceConfig(p.ues), p.R, G, sched=sched)
        cell = oracle.Cell(p.ues, p.R, G, sched)
        kw, ids, out = one_call(oracle, cell, p)
        check_plain(p, eff, out)
        same_call(ts.schedule_tti(**kw), out, ids, f"sched {sched} {p.name}", upper=sched == 10)
        if sched not in (1, 7):
            kw, ids, out = one_call(oracle, cell, p, subset_ids(p))
            check_plain(p, eff, out, ids)
            same_call(ts.schedule_tti(**kw), out, ids, f"sched {sched} {p.name}, subset call", upper=sched == 10)
        ts.close()


@pytest.mark.parametrize("sched", [101, 103])
def test_dropin_calls_of_the_other_inter_slice_steps(rs, oracle, eff, sched):
    p = nt.transport_set(eff, sched)[3]
    ts = rs.TtiScheduler(rs.SliceConfig(p.ues), p.R, 4, sched=sched)
    cell = oracle.Cell(p.ues, p.R, 4, sched)
    kw, ids, out = one_call(oracle, cell, p)
    check_plain(p, eff, out)
    same_call(ts.schedule_tti(**kw), out, ids, f"sched {sched} {p.name}")
    ts.close()


def test_dropin_per_prb_reports(rs, oracle, eff):
    for p in nt.transport_set(eff, 9)[:4]:
        G = rbg_size(p.R)
        ts = rs.TtiScheduler(rs.SliceConfig(p.ues), p.R, G, sched=9)
        cell = oracle.Cell(p.ues, p.R, G, 9)
        kw, ids, out = one_call(oracle, cell, p, per_prb=True)
        check_plain(p, eff, out)
        same_call(ts.schedule_tti(**kw), out, ids, f"sched 9 {p.name}, per-PRB reports")
        ts.close()


@pytest.mark.parametrize("sched", [9, 1, 7])
def test_dropin_runtime_builds(rs, oracle, eff, sched):
    """The context's own build (rs_ctx_specialize; jit=True at creation is the Python route to it, so the built-in kernel of the same
    shape is test_dropin_calls'), its first-calls self-check left on: the R = 8 populations of one shape, the subset
    call and the exact-scan case; the build must still serve afterwards."""
    pops = [p for p in pops_of(eff, sched) if p.R == 8 and p.ues == pops_of(eff, sched)[0].ues]
    assert len(pops) >= 3 and any("exact-scan" in p.name for p in pops)
    p0 = pops[0]
    ts = rs.TtiScheduler(rs.SliceConfig(p0.ues), 8, 4, sched=sched, jit=True)
    cell = oracle.Cell(p0.ues, 8, 4, sched)
    for rnd in range(2):   # twice: the later calls run without the built-in kernel beside them
        for p in pops:
            kw, ids, out = one_call(oracle, cell, p)
            same_call(ts.schedule_tti(**kw), out, ids, f"sched {sched} {p.name}, run-time build, round {rnd}")
            if sched == 9:
                kw, ids, out = one_call(oracle, cell, p, subset_ids(p))
                same_call(ts.schedule_tti(**kw), out, ids, f"sched {sched} {p.name}, run-time build, subset call")
    assert ts.jit_status()[0] == 1, ts.jit_status()
    ts.close()


# ---------------------------------------------------------------------------------------------------------------------------
# group calls
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sched", [9, 1, 7])
def test_group_calls_plain_and_resident(rs, oracle, eff, sched):
    """Three cells, a population each.  Plain form: one launch.  Resident form: set_avg with the near-tie averages, one call at
    now == last_update (the averages are used as given), then 45 TTIs with constant reports on the device's own EWMA, against the
    oracle stepped the same way: every output field of every TTI, and the averages after TTIs 1, 20 and 45."""
    pops = nt.group_set(eff, sched)
    K, R, G = len(pops), 8, 4
    ues = pops[0].ues
    sc = rs.SliceConfig(ues)
    u2s = np.asarray(sc.user_to_slice)
    g = rs.GroupScheduler(sc, R, G, K, sched=sched)
    cells = [oracle.Cell(ues, R, G, sched) for _ in range(K)]
    calls, outs, ids = [], [], None
    for k, p in enumerate(pops):
        kw, ids, out = one_call(oracle, cells[k], p)
        check_plain(p, eff, out)
        calls.append(kw)
        outs.append(out)
    res = g.schedule_tti(calls)
    for k in range(K):
        same_call(res[k], outs[k], ids, f"group sched {sched} cell {k} ({pops[k].name})")
    # resident: the averages as given
    for k, p in enumerate(pops):
        g.set_avg(k, p.avg, 0.1)
    res = g.schedule_tti_at([{x: v for x, v in c.items() if x != "avg_rate"} for c in calls], 0.1)
    for k in range(K):
        same_call(res[k], outs[k], ids, f"group sched {sched} cell {k}, resident call at now == last_update")
    g.close()
    # resident: 45 TTIs on the device's own averages (a fresh group and fresh oracle cells: the first call above recorded grants)
    g = rs.GroupScheduler(sc, R, G, K, sched=sched)
    cells = [oracle.Cell(ues, R, G, sched) for _ in range(K)]
    for k, p in enumerate(pops):
        cells[k].set_cqi(p.cqi)
        cells[k].set_avg_rate(p.avg)
        cells[k].set_last_update(0.1)
        g.set_avg(k, p.avg, 0.1)
    ticks = oracle.clock_ticks(100, 45)
    rands = [oracle.Rng(900 + k) for k in range(K)]
    changed = 0
    prev = [None] * K
    for it in range(45):
        calls, outs, ids_of = [], [], []
        for k, p in enumerate(pops):
            r0, r1 = rands[k].rand(), rands[k].rand()
            out = cells[k].new_out()
            assert cells[k].step(float(ticks[it]), r0, r1, out) == 0
            kw = dict(cqi=p.cqi, rand0=r0, rand1=r1, cqi_epoch=1)
            tti_ids = None
            if sched == 7:
                tti_ids = np.flatnonzero(u2s == out.served_slice).astype(np.int32)
                kw.update(cqi=p.cqi[tti_ids], user_id=tti_ids, cqi_epoch=0)
            calls.append(kw)
            outs.append(out)
            ids_of.append(tti_ids)
            changed += int(prev[k] is not None and (prev[k] != out.rbg_to_user).any())
            prev[k] = out.rbg_to_user.copy()
        res = g.schedule_tti_at(calls, ticks[it])
        for k in range(K):
            what = f"group sched {sched} cell {k}, resident TTI {it}"
            if ids_of[k] is None:
                same_call(res[k], outs[k], None, what)
            else:
                _same_by_id(res[k], outs[k], ids_of[k], what)
        if it + 1 in (1, 20, 45):
            for k in range(K):
                assert g.get_avg(k)[0].tobytes() == cells[k].state()["avg_rate"].tobytes(), f"sched {sched} after TTI {it + 1}, cell {k}: averages"
    assert changed > 0, "the winners never changed: the EWMA's near-ties were not exercised"
    g.close()


# ---------------------------------------------------------------------------------------------------------------------------
# batches: held winners and speculation
# ---------------------------------------------------------------------------------------------------------------------------

N_BATCH = (1, 44, 45)   # a hold period (RS_HOLD_MAX_AGE TTIs) ends inside the second launch, another begins


def _batch_reference(oracle, pops, sched, grids, seeds, weights=None):
    logs, states = [], []
    for k, p in enumerate(pops):
        cell = oracle.Cell(p.ues, p.R, 4, sched, weights=weights)
        cell.set_avg_rate(p.avg)
        again = np.concatenate([grids[k], grids[k][:1]])   # (the oracle's run does not wrap: the same grid a third time)
        logs.append(cell.run_synth(again, int(seeds[k]), sum(N_BATCH)))
        states.append(cell.state())
    return logs, states


def _batch_against_the_oracle(rs, oracle, pops, sched, jit, weights=None, logged=True):
    K, R, G = len(pops), 8, 4
    sc = rs.SliceConfig(pops[0].ues, weight=list(weights) if weights else [])
    grids = np.stack([np.stack([p.cqi, p.cqi]) for p in pops])
    seeds = np.arange(K, dtype=np.uint32) + 31
    logs, states = _batch_reference(oracle, pops, sched, grids, seeds, weights)
    b = rs.BatchScheduler(sc, R, G, K, sched=sched, jit=jit, cqi_epoch_wrap=True)
    b.seed(seeds)
    b.upload_cqi_epochs(grids)
    b.write_state(avg_rate=np.stack([p.avg for p in pops]))
    if logged:
        got = [b.run_logged(n) for n in N_BATCH]
    else:
        b.run(sum(N_BATCH))
    st = b.state()
    status = b.jit_status()
    b.close()
    assert status[0] == (1 if jit else 0), status   # a failed build would quietly run the built-in kernel
    what = f"sched {sched} {'run-time build' if jit else 'built-in'}"
    for k in range(K):
        if logged:
            maps = np.concatenate([x["rbg_to_user"] for x in got], axis=1)
            tbs = np.concatenate([x["tbs_bits"] for x in got], axis=1)
            np.testing.assert_array_equal(maps[k], logs[k]["rbg_to_user"], err_msg=f"{what} cell {k}: RBG maps")
            np.testing.assert_array_equal(tbs[k], logs[k]["tbs_bits"], err_msg=f"{what} cell {k}: transport blocks")
        assert st["avg_rate"][k].tobytes() == states[k]["avg_rate"].tobytes(), f"{what} cell {k}: averages"
        assert (st["cum_bytes"][k] == states[k]["cum_bytes"]).all() and (st["cum_rbs"][k] == states[k]["cum_rbs"]).all()
        assert st["slice_state"][k].tobytes() == states[k]["slice_state"].tobytes(), f"{what} cell {k}: slice state"


BATCHES = [(9, False), (8, False), (1, False), (7, False), (10, False), (9, True), (8, True), (1, True), (7, True), (10, True)]


@pytest.mark.parametrize("sched,jit", BATCHES, ids=[f"{s}-{'jit' if j else 'builtin'}" for s, j in BATCHES])
def test_batches(rs, oracle, eff, sched, jit):
    """Two cells with near-tie averages (write_state), two identical CQI epochs, 1 + 44 + 45 logged TTIs: RBG maps and transport
    blocks of every TTI, final averages, counters and slice state against the oracle's run.  Scheduler 7's slice 1 is scanned in
    runs here, with pairs either side of the run boundaries (near_ties.batch_set)."""
    _batch_against_the_oracle(rs, oracle, nt.batch_set(eff, sched), sched, jit)


MARGINS = [(9, True), (8, True), (9, False), (8, False)]


@pytest.mark.parametrize("sched,jit", MARGINS, ids=[f"{s}-{'jit' if j else 'builtin'}" for s, j in MARGINS])
def test_batches_around_the_hold_margin(rs, oracle, eff, sched, jit):
    """The held-winner rule (run-time builds of schedulers 8 and 9) on near_ties.margin_population: winners of average 64, 65, 1e3,
    1e5 with runner-ups 0.5 ... 2 mu behind, in slices that starve.  tests/test_near_tie_inputs.py shows that 8 of the 32 items
    pass the held test at the full scan and that winners change within RS_HOLD_MAX_AGE TTIs of it."""
    _batch_against_the_oracle(rs, oracle, [nt.margin_population(eff, sched)], sched, jit, weights=nt.MARGIN_WEIGHTS)


def test_batch_unlogged_lean_build(rs, oracle, eff, monkeypatch):
    monkeypatch.setenv("RS_JIT_LEAN_MIN_TTIS", "1")
    _batch_against_the_oracle(rs, oracle, nt.batch_set(eff, 9), 9, True, logged=False)
    _batch_against_the_oracle(rs, oracle, [nt.margin_population(eff, 9)], 9, True, weights=nt.MARGIN_WEIGHTS, logged=False)


# ---------------------------------------------------------------------------------------------------------------------------
# scheduler 1's flows form
# ---------------------------------------------------------------------------------------------------------------------------

def test_group_flows_form(rs, oracle, eff):
    """Three flow-resident cells (set_flows) of 40 users with two InfiniteBuffer bearers each: a user's two bearers a near-tie apart
    in both orders, neighbouring users' flows at positions 31|32 and 63|64, 45 TTIs of schedule_tti_flows against the oracle's queue
    path (rso_cell_step_queues) started from the same averages; rbg_to_user (flow ids) and per-user sums every TTI, every bearer's
    average after TTIs 1, 20 and 45."""
    from test_gpu_group_flows import same_as_oracle
    U, R, G, K = nt.FLOW_USERS, 8, 4, len(nt.GROUP_AVGS)
    pops = [nt.flows_population(eff, a, 300 + k) for k, a in enumerate(nt.GROUP_AVGS)]
    g = rs.GroupScheduler(rs.SliceConfig([2 * U]), R, G, K, sched=1)
    cells, rngs = [], []
    has = np.zeros((2 * U, 2), bool)
    has[:U] = True
    for k, (cqi, avg2, _) in enumerate(pops):
        cell = oracle.Cell([U], R, G, 1)
        cell.enable_queues(np.ones((U, 2), np.uint8))
        cell.set_bearer_avg(avg2)
        cell.set_cqi(cqi)
        cells.append(cell)
        rngs.append(oracle.Rng(77 + k))
        pad = np.zeros((2 * U, 2))
        pad[:U] = avg2
        g.set_flows(k, has, pad, LAST0)
    uid = np.repeat(np.arange(U, dtype=np.int32), 2)
    fb = np.tile(np.array([0, 1], np.uint8), U)
    ticks = oracle.clock_ticks(100, 45)
    for t in range(45):
        outs = []
        for k in range(K):
            out = cells[k].new_out()
            assert cells[k].step_queues(float(ticks[t]), rngs[k], out) == 0
            outs.append(out)
        res = g.schedule_tti_flows([dict(user_id=uid, flow_bearer=fb, data_to_transmit=np.full(2 * U, INFINITE, np.int32),
                                         cqi=p[0][uid], cqi_epoch=1) for p in pops], ticks[t])
        for k in range(K):
            same_as_oracle(res[k], dict(out=outs[k], uid=uid), f"flows TTI {t} cell {k}")
        if t + 1 in (1, 20, 45):
            for k in range(K):
                assert g.get_flows(k)[0][:U].tobytes() == cells[k].bearer_state()["avg_rate"].tobytes(), f"flows after TTI {t + 1}, cell {k}: averages"
    g.close()
