"""The quota step (P2) and scheduler 7's slice pick on the directed inputs of tests/quota_edges.py: truncation after one rounding,
products that a fused multiply-add would round differently, negative extras and remainders, every rotation head, quota vectors with
negative entries, zeros and entries above R, offsets carried over 8 TTIs, and EWMA scores that are equal, an ulp apart, either side
of the low word's sign bit, infinite, or held by empty slices.  tests/test_quota_edge_inputs.py proves on the CPU that the cases bind
and that the oracle equals the plain model on them; here the kernels meet them on every surface that runs the step: drop-in calls
(built-in and run-time builds, subset calls), group calls (plain, resident, T-TTI runs and their run-time build) and batches (the
speculated and held-winner halves of the step, scheduler 7's picks made a TTI ahead).  Every comparison is bitwise: device == oracle
on every output field, and targets and quotas == the plain model.

Found by these tests: no difference in the kernels.  Writing them showed that every surface hands targets and quotas out as int16,
so an offset of magnitude 2^15 came back as a wrong target long before idiv_small's exact range (below 2^25 + 2) ends; the three
setters of the slice state took any double.  They now refuse non-finite values, offsets that could carry a target to 2^15, and
negative EWMAs (test_setters_refuse_what_the_quota_step_cannot_handle)."""
import numpy as np
import pytest

import quota_edges as qe
from test_gpu_dropin_oracle import same_call
from test_quota_edge_inputs import ONE_CALL, arrays, case_ids, granted_of, oracle_case_call, oracle_cell

pytestmark = pytest.mark.gpu

A_SHAPE, B_SHAPE = ((3, 2, 4, 3), 25, 4), ((3, 2, 3), 8, 4)     # the two shapes that also get run-time builds


def one_call_cases():
    return [c for f in ONE_CALL for c in qe.cases(f)]


def report(what, cs):
    n = {f: sum(1 for c in cs if c.family == f) for f in qe.FAMILIES}
    print(f"quota edge cases run, {what}: " + ", ".join(f"{f} {n[f]}" for f in qe.FAMILIES if n[f]))
    for f in {c.family for c in cs}:
        assert n[f] == len(qe.cases(f)), f"{what}: {n[f]} of {len(qe.cases(f))} {f} cases"


def config_of(rs, c):
    return rs.SliceConfig(list(c.ues), weight=list(c.w))


def call_kw(c):
    cqi, avg = arrays(c)
    ids = case_ids(c)
    rows = slice(None) if ids is None else ids
    kw = dict(cqi=cqi[rows], avg_rate=avg[rows], rand0=c.r0, rand1=c.r1)
    if ids is not None:
        kw["user_id"] = ids
    return kw


def check_call(res, out, c, sched, what, offset=None, r0=None, r1=None):
    """device == oracle on every field; targets and quotas == the plain model; scheduler 8's map == plain GreedyByRow"""
    same_call(res, out, case_ids(c), what, upper=sched == 10)
    target, quota = qe.plain_quotas(c.nb, c.G, c.w, c.state if offset is None else offset, c.has, c.r0 if r0 is None else r0,
                                    c.r1 if r1 is None else r1)
    assert res.target_rbs.tolist() == target, f"{what}: targets against the plain model"
    assert res.quota_rbgs.tolist() == quota, f"{what}: quotas against the plain model"
    if sched == 8:
        u2s = np.array(c.u2s)
        got = [int(u2s[u]) if u >= 0 else -1 for u in res.rbg_to_user]
        assert got == qe.plain_greedy_by_row(out.slice_eff.tolist(), quota), f"{what}: RBG-to-slice map against the plain model"
    return target


# ---------------------------------------------------------------------------------------------------------------------------
# drop-in calls
# ---------------------------------------------------------------------------------------------------------------------------

def _dropin(rs, oracle, sched, cs, jit):
    for group in qe.by_config(cs):
        ts = rs.TtiScheduler(config_of(rs, group[0]), group[0].R, group[0].G, sched=sched, jit=jit)
        for rnd in range(2 if jit else 1):    # (a run-time build's first calls run beside the built-in kernel)
            for c in group:
                what = f"sched {sched} {'run-time build' if jit else 'built-in'} {c.name}"
                cell = oracle_cell(oracle, c, sched)
                out = oracle_case_call(oracle, cell, c)
                ts.slice_offset = c.state
                res = ts.schedule_tti(**call_kw(c))
                target = check_call(res, out, c, sched, what)
                after = ts.slice_offset
                assert after.tobytes() == cell.state()["slice_state"].tobytes(), f"{what}: slice offsets afterwards"
                assert after.tolist() == qe.plain_offsets_after(target, granted_of(c, sched, out), c.G), f"{what}: offsets against the plain model"
        if jit:
            assert ts.jit_status()[0] == 1, ts.jit_status()
        ts.close()


@pytest.mark.parametrize("sched", qe.TRANSPORT)
def test_dropin_calls(rs, oracle, sched):
    """Every trunc, product, negdiv, rotate and policy case through the built-in kernel: slice_offset set, one call with the case's
    rands (a subset call where the case lists its users), every output field, slice_offset afterwards."""
    cs = one_call_cases()
    _dropin(rs, oracle, sched, cs, False)
    report(f"drop-in sched {sched}", cs)


@pytest.mark.parametrize("sched", [9, 8, 103])
def test_dropin_runtime_builds(rs, oracle, sched):
    """The context's own build on the cases of two shapes (12 users on 25 x 4, 8 users on 8 x 4), twice over"""
    cs = [c for c in one_call_cases() if c.shape in (A_SHAPE, B_SHAPE)]
    assert {c.shape for c in cs} == {A_SHAPE, B_SHAPE} and {c.family for c in cs} == set(ONE_CALL)
    _dropin(rs, oracle, sched, cs, True)


# ---------------------------------------------------------------------------------------------------------------------------
# group calls
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sched", [9, 101])
def test_group_calls_plain_and_resident(rs, oracle, sched):
    """One group per configuration, one case per cell: set_slice_offset, one plain launch; the offsets again, set_avg, one resident
    launch at now == last_update (the averages are used as given)."""
    cs = one_call_cases()
    for group in qe.by_config(cs):
        K = len(group)
        g = rs.GroupScheduler(config_of(rs, group[0]), group[0].R, group[0].G, K, sched=sched)
        cells = [oracle_cell(oracle, c, sched) for c in group]
        outs = [oracle_case_call(oracle, cells[k], c) for k, c in enumerate(group)]
        for form in ("plain", "resident"):
            calls = [call_kw(c) for c in group]
            for k, c in enumerate(group):
                g.set_slice_offset(k, c.state)
            if form == "plain":
                res = g.schedule_tti(calls)
            else:
                for k, c in enumerate(group):
                    g.set_avg(k, arrays(c)[1], 0.1)
                    del calls[k]["avg_rate"]
                res = g.schedule_tti_at(calls, 0.1)
            for k, c in enumerate(group):
                what = f"group sched {sched} {form} {c.name}"
                check_call(res[k], outs[k], c, sched, what)
                assert g.slice_offset(k).tobytes() == cells[k].state()["slice_state"].tobytes(), f"{what}: slice offsets afterwards"
        g.close()
    report(f"group sched {sched}", cs)


def _chain_runs(rs, oracle, sched, cs, jit_run):
    T = qe.CHAIN_TTIS
    ticks = oracle.clock_ticks(100, T)
    for group in qe.by_config(cs):
        K = len(group)
        g = rs.GroupScheduler(config_of(rs, group[0]), group[0].R, group[0].G, K, sched=sched, jit_run=jit_run)
        for rnd in range(2 if jit_run else 1):
            cells = []
            for k, c in enumerate(group):
                cqi, avg = arrays(c)
                cell = oracle_cell(oracle, c, sched)
                cell.set_cqi(cqi)
                cell.set_avg_rate(avg)
                cell.set_last_update(0.1)
                cells.append(cell)
                g.set_slice_offset(k, c.state)
                g.set_avg(k, avg, 0.1)
            res = g.run_at([dict(cqi=arrays(c)[0], cqi_epoch=1 + rnd) for c in group], ticks, np.array([c.rands for c in group], np.int32))
            for k, c in enumerate(group):
                before = list(c.state)
                flips = 0
                for t in range(T):
                    what = f"run sched {sched}{' run-time build' if jit_run else ''} {c.name} TTI {t}"
                    out = cells[k].new_out()
                    r0, r1 = c.rands[t]
                    assert cells[k].step(float(ticks[t]), r0, r1, out) == 0
                    check_call(res[k][t], out, c, sched, what, offset=before, r0=r0, r1=r1)
                    after = cells[k].state()["slice_state"].tolist()
                    flips += sum(1 for a, b in zip(before, after) if a * b < 0)
                    before = after
                assert flips > 0, f"{c.name}: no offset changed sign"
                assert g.slice_offset(k).tobytes() == cells[k].state()["slice_state"].tobytes(), f"run sched {sched} {c.name}: offsets afterwards"
        if jit_run:
            assert g.run_jit_status()[0] == 1, g.run_jit_status()
        g.close()


@pytest.mark.parametrize("sched", [8, 9, 10, 103])
def test_group_runs_carry_the_offsets(rs, oracle, sched):
    """The chain cases through run_at: 8 TTIs in one launch on constant reports and the case's rands, the offsets carried in the
    kernel, against the oracle stepped 8 times: every field of every TTI, the offsets afterwards."""
    cs = qe.cases("chain")
    _chain_runs(rs, oracle, sched, cs, False)
    report(f"group runs sched {sched}", cs)


def test_group_runs_runtime_build(rs, oracle):
    cs = [c for c in qe.cases("chain") if c.shape == A_SHAPE]
    assert len(cs) >= 2
    _chain_runs(rs, oracle, 9, cs, True)


# ---------------------------------------------------------------------------------------------------------------------------
# batches
# ---------------------------------------------------------------------------------------------------------------------------

BATCH_FAMILIES = ("product", "negdiv", "chain")
BATCH_TTIS = (1, 7)
SEED0 = 4100


def _batch(rs, oracle, sched, group, jit):
    """One batch of len(group) cells, cell k started from case k: offsets and averages through write_state, two identical CQI epochs,
    1 + 7 logged TTIs on the batch's own rand() streams"""
    K, c0 = len(group), group[0]
    n = sum(BATCH_TTIS)
    has = [u > 0 for u in c0.ues]     # (a batch schedules every user: the cases' subset lists do not apply)
    seeds = np.arange(K, dtype=np.uint32) + SEED0
    b = rs.BatchScheduler(config_of(rs, c0), c0.R, c0.G, K, sched=sched, jit=jit, cqi_epoch_wrap=True)
    b.seed(seeds)
    b.upload_cqi_epochs(np.stack([np.stack([arrays(c)[0]] * 2) for c in group]))
    b.write_state(avg_rate=np.stack([arrays(c)[1] for c in group]), slice_state=np.array([c.state for c in group]))
    logs = [b.run_logged(t) for t in BATCH_TTIS]
    st = b.state()
    status = b.jit_status()
    b.close()
    assert status[0] == (1 if jit else 0), status
    quota = np.concatenate([x["quota"] for x in logs], axis=1)
    target = np.concatenate([x["target"] for x in logs], axis=1)
    maps = np.concatenate([x["rbg_to_user"] for x in logs], axis=1)
    tbs = np.concatenate([x["tbs_bits"] for x in logs], axis=1)
    ticks = oracle.clock_ticks(100, n)
    for k, c in enumerate(group):
        cqi, avg = arrays(c)
        cell = oracle_cell(oracle, c, sched)
        cell.set_cqi(cqi)
        cell.set_avg_rate(avg)
        cell.set_last_update(0.1)
        rng = oracle.Rng(int(seeds[k]))
        before = list(c.state)
        for t in range(n):
            what = f"batch sched {sched} {'run-time build' if jit else 'built-in'} {c.name} TTI {t}"
            r0, r1 = rng.rand(), rng.rand()
            out = cell.new_out()
            assert cell.step(float(ticks[t]), r0, r1, out) == 0
            want_t, want_q = qe.plain_quotas(c.nb, c.G, c.w, before, has, r0, r1)
            assert target[k, t].tolist() == out.target_rbs.tolist() == want_t, f"{what}: targets"
            assert quota[k, t].tolist() == out.quota_rbgs.tolist() == want_q, f"{what}: quotas"
            np.testing.assert_array_equal(maps[k, t], out.rbg_to_user, err_msg=f"{what}: RBG map")
            np.testing.assert_array_equal(tbs[k, t], out.user_tbs_bits, err_msg=f"{what}: transport blocks")
            before = cell.state()["slice_state"].tolist()
        assert st["slice_state"][k].tobytes() == cell.state()["slice_state"].tobytes(), f"batch sched {sched} {c.name}: final slice state"
        assert st["avg_rate"][k].tobytes() == cell.state()["avg_rate"].tobytes(), f"batch sched {sched} {c.name}: final averages"


BATCHES = [(9, False), (8, False), (10, False), (101, False), (103, False), (9, True), (8, True)]


@pytest.mark.parametrize("sched,jit", BATCHES, ids=[f"{s}-{'jit' if j else 'builtin'}" for s, j in BATCHES])
def test_batches(rs, oracle, sched, jit):
    """The product, negdiv and chain starts: per-TTI quota and target against the plain model and the oracle, maps, transport
    blocks, final slice state.  Schedulers 9 and 8 run the quota step a TTI early on another wave (speculation; held winners in
    their run-time builds); the run-time builds take the cases of the 12-user 25 x 4 shape (one build per scheduler)."""
    cs = [c for f in BATCH_FAMILIES for c in qe.cases(f)]
    if jit:
        cs = [c for c in cs if c.shape == A_SHAPE]
        assert {c.family for c in cs} == set(BATCH_FAMILIES)
    for group in qe.by_config(cs):
        _batch(rs, oracle, sched, group, jit)
    if not jit:
        report(f"batches sched {sched}", cs)


N3_SHAPE = ((2, 2, 2), 8, 4)
NVS_TTIS = (1, 1, 4)


@pytest.mark.parametrize("jit", [False, True], ids=["builtin", "jit"])
def test_sched7_batches(rs, oracle, jit):
    """The nvs cases: EWMAs through write_state, 6 logged TTIs in launches of 1, 1 and 4 (picks made a TTI ahead are among them):
    the served slice of every TTI, read from rbg_to_user through user_to_slice, and slice_state after 1, 2 and 6 TTIs, against the
    oracle and plain_nvs_pick.  The run-time build takes the cases of the three-slice shape."""
    cs = qe.cases("nvs")
    if jit:
        cs = [c for c in cs if c.shape == N3_SHAPE]
        assert len(cs) >= 12
    ticks = oracle.clock_ticks(100, sum(NVS_TTIS))
    for group in qe.by_config(cs):
        K, c0 = len(group), group[0]
        b = rs.BatchScheduler(config_of(rs, c0), c0.R, c0.G, K, sched=7, jit=jit, cqi_epoch_wrap=True)
        b.seed(np.arange(K, dtype=np.uint32) + SEED0)
        b.upload_cqi_epochs(np.stack([np.stack([arrays(c)[0]] * 2) for c in group]))
        b.write_state(avg_rate=np.stack([arrays(c)[1] for c in group]), slice_state=np.array([c.state for c in group]))
        cells, ewma = [], [list(c.state) for c in group]
        for c in group:
            cell = oracle.Cell(c.ues, c.R, c.G, oracle.SCHED_NVS, weights=c.w)
            cell.set_slice_offset(c.state)
            cell.set_cqi(arrays(c)[0])
            cell.set_avg_rate(arrays(c)[1])
            cell.set_last_update(0.1)
            cells.append(cell)
        t = 0
        for n in NVS_TTIS:
            log = b.run_logged(n)
            for j in range(n):
                for k, c in enumerate(group):
                    what = f"sched 7 {'run-time build' if jit else 'built-in'} {c.name} TTI {t}"
                    out = cells[k].new_out()
                    assert cells[k].step(float(ticks[t]), 0, 0, out) == 0
                    pick, ewma[k] = qe.plain_nvs_pick(c.w, ewma[k], c.has)
                    m = log["rbg_to_user"][k, j]
                    np.testing.assert_array_equal(m, out.rbg_to_user, err_msg=f"{what}: RBG map")
                    served = {c.u2s[u] for u in m if u >= 0}
                    assert served == {pick} and out.served_slice == pick, f"{what}: served slice {served}, plain model {pick}"
                    np.testing.assert_array_equal(log["tbs_bits"][k, j], out.user_tbs_bits, err_msg=f"{what}: transport blocks")
                t += 1
            st = b.state()["slice_state"]
            for k, c in enumerate(group):
                want = np.array(ewma[k], np.float64)
                assert st[k].tobytes() == cells[k].state()["slice_state"].tobytes() == want.tobytes(), f"sched 7 {c.name}: EWMAs after {t} TTIs"
        status = b.jit_status()
        b.close()
        assert status[0] == (1 if jit else 0), status
    if not jit:
        report("sched 7 batches", cs)


# ---------------------------------------------------------------------------------------------------------------------------
# the setters' domain
# ---------------------------------------------------------------------------------------------------------------------------

def _refused(rs, fn, *args):
    with pytest.raises(rs.RadioSaberError) as e:
        fn(*args)
    assert e.value.code == -1 and str(e.value), str(e.value)     # RS_ERR_INVALID with a message


BAD_OFFSETS = [[np.nan, 0, 0, 0], [0, np.inf, 0, 0], [0, 0, -np.inf, 0], [0, 0, 0, 2.0**15], [-15900.0, 15900.0, 0, 0], [0, -1e300, 0, 0],
               [2.0**25 + 2 - 100, 0, 0, 0]]                # (the last: idiv_small's bound less nb_rbs)
GOOD_OFFSETS = [15800.0, -15900.0, 0.5, -0.0]               # 5 * 100 * (1 + 1) + sum |offset| = 32700.5 < 2^15
BAD_EWMAS = [[np.nan, 0, 0, 0], [0.5, -1e-300, 0, 0], [0, 0, np.inf, 0], [0, 0, 0, -1.0]]


def test_setters_refuse_what_the_quota_step_cannot_handle(rs):
    """rs_set_slice_offset, rs_group_set_slice_offset and rs_batch_write_state: non-finite values, offsets that could carry a target
    past the int16 the outputs hold it in -- a bound far inside the one at which the step's divisions stop being exact
    (include/radiosaber_hip.h) --, negative EWMAs for scheduler 7.  A refused call leaves the state as it was; the largest accepted
    offsets are taken.  (Before, all three setters took any double.)"""
    ues, R, G = [3, 2, 4, 3], 25, 4
    sc = rs.SliceConfig(ues, weight=[0.25] * 4)
    start = np.array([1.5, -2.0, 0.0, 3.0])
    for sched, bad in ((9, BAD_OFFSETS), (8, BAD_OFFSETS), (7, BAD_EWMAS)):
        first = np.abs(start) if sched == 7 else start
        ts = rs.TtiScheduler(sc, R, G, sched=sched)
        ts.slice_offset = first
        g = rs.GroupScheduler(sc, R, G, 2, sched=sched)
        g.set_slice_offset(1, first)
        b = rs.BatchScheduler(sc, R, G, 2, sched=sched)
        b.write_state(slice_state=np.stack([first, first]))
        for v in bad:
            v = np.array(v, np.float64)
            _refused(rs, lambda: setattr(ts, "slice_offset", v))
            _refused(rs, g.set_slice_offset, 1, v)
            _refused(rs, lambda: b.write_state(slice_state=np.stack([first * 2, v])))    # (cell 0's values are fine: nothing is written)
            assert ts.slice_offset.tobytes() == first.tobytes()
            assert g.slice_offset(1).tobytes() == first.tobytes() and not g.slice_offset(0).any()
            assert b.state()["slice_state"].tobytes() == np.stack([first, first]).tobytes()
        good = np.array([1e300, 0.0, 5e-324, 1.0]) if sched == 7 else np.array(GOOD_OFFSETS)
        ts.slice_offset = good
        g.set_slice_offset(0, good)
        b.write_state(slice_state=np.stack([good, first]))
        assert ts.slice_offset.tobytes() == g.slice_offset(0).tobytes() == b.state()["slice_state"][0].tobytes() == good.tobytes()
        ts.close()
        g.close()
        b.close()
    # scheduler 1 keeps no slice state of its own: any finite value passes, a NaN does not
    b = rs.BatchScheduler(sc, R, G, 1, sched=1)
    b.write_state(slice_state=np.array([[-1e300, 2.0**40, 0, 0]]))
    _refused(rs, lambda: b.write_state(slice_state=np.array([[np.nan, 0, 0, 0]])))
    b.close()


def test_the_largest_accepted_offsets_come_back_whole(rs, oracle):
    """Two calls at the edge of the setters' domain: targets of +-15850 PRBs and quotas of +-3962 RBGs, then the call that reads the
    offsets these leave behind; device == oracle == plain model, nothing lost in the int16 outputs."""
    c = qe._mk("largest accepted offsets", "trunc", qe.A, qe.W4, GOOD_OFFSETS, r0=5, r1=6)
    for sched in (9, 8):
        cell = oracle_cell(oracle, c, sched)
        out = oracle_case_call(oracle, cell, c)
        ts = rs.TtiScheduler(config_of(rs, c), c.R, c.G, sched=sched)
        ts.slice_offset = c.state
        res = ts.schedule_tti(**call_kw(c))
        target = check_call(res, out, c, sched, f"sched {sched} {c.name}")
        assert max(abs(t) for t in target) > 15000
        after = cell.state()["slice_state"]
        assert ts.slice_offset.tobytes() == after.tobytes()
        out = oracle_case_call(oracle, cell, c, 7, 8)
        res = ts.schedule_tti(**dict(call_kw(c), rand0=7, rand1=8))
        check_call(res, out, c, sched, f"sched {sched} {c.name}, the call after", offset=after.tolist(), r0=7, r1=8)
        assert ts.slice_offset.tobytes() == cell.state()["slice_state"].tobytes()
        ts.close()
