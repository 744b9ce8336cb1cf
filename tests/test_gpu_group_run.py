"""rs_group_run_at / GroupScheduler.run_at: T consecutive TTIs of average-resident cells in one launch.  The call is defined as a loop of
rs_group_schedule_tti_at calls, so the expectation is a twin group fed the same TTIs one call at a time, and the oracle's own DoSchedule
loop where the oracle restates the scheduler.  Every comparison is bitwise."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import synth_cqi
from test_gpu_group import HIST, _same

pytestmark = pytest.mark.gpu

UES, R, G, K = [5, 4, 3], 8, 2, 3      # 3 cells; slices of 5 / 4 / 3 users; 8 RBGs of 2 PRBs
W = [0.5, 0.3, 0.2]
RUN_SCHEDS = (1, 8, 9, 10, 101, 103)


def _pairs(rng, n, T):
    return rng.integers(0, 2**31 - 1, (n, T, 2)).astype(np.int32)


def _calls(n_cells, U, seed, epoch, n_rbgs=R, **kw):
    return [dict(cqi=synth_cqi(seed + k, (U, n_rbgs), HIST), cqi_epoch=epoch, **kw) for k in range(n_cells)]


def _one_at_a_time(twin, calls, nows, rands, cell_ids=None):
    """What a run is defined as: T schedule_tti_at calls on `twin`; results[k][t]."""
    n = len(calls)
    nows = np.broadcast_to(np.asarray(nows, np.float64), (n, np.shape(nows)[-1]))
    res = [[] for _ in range(n)]
    for t in range(nows.shape[1]):
        step = twin.schedule_tti_at([dict(c, rand0=int(rands[k, t, 0]), rand1=int(rands[k, t, 1])) for k, c in enumerate(calls)], nows[:, t],
                                    cell_ids=cell_ids)
        for k in range(n):
            res[k].append(step[k])
    return res


def _state(g, n_cells):
    """Everything a test can read of the cells: averages, pending bytes, last_update, slice offsets -- as bytes."""
    out = []
    for k in range(n_cells):
        a, pend, last = g.get_avg(k)
        out.append((a.tobytes(), pend.tobytes(), last, g.slice_offset(k).tobytes()))
    return out


def _same_runs(res, ref, what, upper=False):
    assert len(res) == len(ref)
    for k, (row, want) in enumerate(zip(res, ref)):
        assert len(row) == len(want)
        for t, (a, b) in enumerate(zip(row, want)):
            _same(a, b, f"{what}: slot {k}, TTI {t}", upper=upper)


def _pair_of_groups(rs, sched, seed, ues=UES, w=W, n_rbgs=R, n_cells=K, last=0.1, **kw):
    sc = rs.SliceConfig(ues, weight=w)
    g = rs.GroupScheduler(sc, n_rbgs, G, n_cells, sched=sched, **kw)
    twin = rs.GroupScheduler(sc, n_rbgs, G, n_cells, sched=sched)
    rng = np.random.default_rng(seed)
    for k in range(n_cells):
        a0 = rng.uniform(1e3, 5e6, sc.n_users)
        g.set_avg(k, a0, last)
        twin.set_avg(k, a0, last)
    return sc, g, twin, rng


# ---------------------------------------------------------------------------------------------------------------------------
# 1. a run is T calls
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [1, 2, 7])
@pytest.mark.parametrize("sched", RUN_SCHEDS)
def test_a_run_is_T_calls(rs, sched, T):
    """Three runs in a row, new grids and a new cqi_epoch before each: every output field of every (cell, TTI) -- scheduler 10 with its
    upper_* lists --, after each run the averages, pending bytes, last_update, slice offsets and image_stats; 3 launches against 3 T."""
    sc, g, twin, rng = _pair_of_groups(rs, sched, 100 * sched + T)
    now = 0.1
    for run in range(3):
        calls = _calls(K, sc.n_users, 1000 * sched + 10 * run + T, epoch=1 + run)
        nows = now + 0.001 * np.arange(1, T + 1)
        now = float(nows[-1])
        rands = _pairs(rng, K, T)
        res = g.run_at(calls, nows, rands)
        ref = _one_at_a_time(twin, calls, nows, rands)
        _same_runs(res, ref, f"sched {sched} T {T} run {run}", upper=sched == 10)
        assert _state(g, K) == _state(twin, K), f"sched {sched} T {T}: state after run {run}"
        assert g.get_avg(0)[2] == now
        assert g.image_stats == twin.image_stats == ((run + 1) * K * (T - 1), (run + 1) * K, 0)
    assert (g.launch_count, twin.launch_count) == (3, 3 * T)
    g.close()
    twin.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. - 4. against the oracle's own DoSchedule loop
# ---------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _oracle_runs(sched, ues, w, n_rbgs, n_cells, n_runs, T, seed):
    """The oracle's side of a run test, computed once per case and shared: per run the grids, the clock and the rand() pairs the run is
    given, the oracle's outputs per (cell, TTI) and its averages behind the run; and the starting averages."""
    from oracle import oracle_py as oracle
    U = sum(ues)
    cells = [oracle.Cell(list(ues), n_rbgs, G, sched, weights=list(w)) for _ in range(n_cells)]
    ticks = oracle.clock_ticks(100, n_runs * T)
    rngs = [oracle.Rng(seed + 17 * k) for k in range(n_cells)]   # (the glibc rand() restatement)
    rng = np.random.default_rng(seed)
    a0 = [rng.uniform(1e3, 5e6, U) for _ in range(n_cells)]
    for k in range(n_cells):   # bearers created at 0.1 s as in the reference's runs
        cells[k].set_avg_rate(a0[k])
        cells[k].set_last_update(0.1)
    runs = []
    for run in range(n_runs):
        grids = [synth_cqi(seed + 1000 * k + run, (U, n_rbgs), HIST) for k in range(n_cells)]
        nows = np.asarray(ticks[run * T:(run + 1) * T], np.float64)
        pairs = np.zeros((n_cells, T, 2), np.int32)
        outs = [[] for _ in range(n_cells)]
        for k in range(n_cells):
            cells[k].set_cqi(grids[k])
        for t in range(T):
            for k in range(n_cells):
                pairs[k, t] = rngs[k].rand(), rngs[k].rand()
                out = cells[k].new_out()
                assert cells[k].step(float(nows[t]), int(pairs[k, t, 0]), int(pairs[k, t, 1]), out) == 0
                outs[k].append(out)
        runs.append(dict(grids=grids, nows=nows, rands=pairs, outs=outs, avg=[cells[k].state()["avg_rate"].copy() for k in range(n_cells)]))
    return a0, runs


def _against_the_oracle(rs, sched, ues, w, n_rbgs, n_cells, n_runs, T, seed):
    a0, runs = _oracle_runs(sched, tuple(ues), tuple(w), n_rbgs, n_cells, n_runs, T, seed)
    sc = rs.SliceConfig(list(ues), weight=list(w))
    g = rs.GroupScheduler(sc, n_rbgs, G, n_cells, sched=sched)
    for k in range(n_cells):
        g.set_avg(k, a0[k], 0.1)
    for i, run in enumerate(runs):
        res = g.run_at([dict(cqi=run["grids"][k], cqi_epoch=1 + i) for k in range(n_cells)], run["nows"], run["rands"])
        for k in range(n_cells):
            for t in range(T):
                _same(res[k][t], run["outs"][k][t], f"sched {sched} run {i} cell {k} TTI {t}")
            a, _, last = g.get_avg(k)
            assert a.tobytes() == run["avg"][k].tobytes(), f"sched {sched} after run {i}, cell {k}: averages"
            assert last == run["nows"][-1]
    assert g.launch_count == n_runs
    assert g.image_stats == (n_runs * n_cells * (T - 1), n_runs * n_cells, 0)
    g.close()


CASE2 = dict(ues=UES, w=W, n_rbgs=R, n_cells=K, n_runs=4, T=10)


@pytest.mark.parametrize("sched", [1, 8, 9])
def test_against_the_oracle(rs, oracle, sched):
    """40 TTIs as four runs of 10, oracle.Cell.step per TTI, the clock of the oracle's run loops, rand pairs from the glibc rand()
    restatement: outputs per TTI, averages after each run."""
    _against_the_oracle(rs, sched, seed=7100 + sched, **CASE2)


@pytest.mark.parametrize("sched", [1, 8, 9])
def test_the_oracle_case_is_not_vacuous(oracle, sched):
    """On the case above, on the oracle's side: TTI 1 of the first run differs from TTI 0 in user_tbs_bits or rbg_to_user for at least
    one cell -- a run that replayed TTI 0 would be caught."""
    _, runs = _oracle_runs(sched, tuple(UES), tuple(W), R, K, 4, 10, 7100 + sched)
    outs = runs[0]["outs"]
    assert any(not np.array_equal(outs[k][1].user_tbs_bits, outs[k][0].user_tbs_bits) or
               not np.array_equal(outs[k][1].rbg_to_user, outs[k][0].rbg_to_user) for k in range(K))


def test_more_users_than_threads(rs, oracle):
    """Slices of 350 + 350 users, 4 RBGs, 2 cells, one run of 5: the strided update, gather and credit cover users beyond the workgroup's
    size on every TTI of the run."""
    _against_the_oracle(rs, 9, [350, 350], [0.5, 0.5], 4, 2, 1, 5, 5300)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. users outside the call, and subsets
# ---------------------------------------------------------------------------------------------------------------------------

def test_users_outside_the_call_are_updated_on_every_tti(rs):
    sc, g, twin, rng = _pair_of_groups(rs, 9, 51)
    U, T = sc.n_users, 6
    ids = np.array([0, 2, 3, 5, 8, 9, 11], np.int32)
    others = np.setdiff1d(np.arange(U), ids)
    before = [g.get_avg(k)[0] for k in range(K)]
    calls = [dict(cqi=synth_cqi(510 + k, (len(ids), R), HIST), user_id=ids, cqi_epoch=3) for k in range(K)]
    nows = 0.1 + 0.001 * np.arange(1, T + 1)
    rands = _pairs(rng, K, T)
    _same_runs(g.run_at(calls, nows, rands), _one_at_a_time(twin, calls, nows, rands), "7 of 12 users")
    assert _state(g, K) == _state(twin, K)
    for k in range(K):   # the five that no TTI named: T EWMA steps without bytes, the numpy float64 expression
        want = before[k][others]
        for _ in nows:   # (rate = 0 bytes / dt = 0 whatever dt is)
            want = ((1 - 0.02) * want) + (0.02 * 0.0)
            want = np.where(want < 1, 1.0, want)
        assert g.get_avg(k)[0][others].tobytes() == want.tobytes(), f"cell {k}: the users outside the call"
        assert (g.get_avg(k)[0][others] != before[k][others]).all()
    g.close()
    twin.close()


def test_a_subset_leaves_the_other_cell_alone(rs):
    sc, g, twin, rng = _pair_of_groups(rs, 9, 52)
    U, T = sc.n_users, 4
    first = _calls(K, U, 520, epoch=5, rand0=11, rand1=12)
    for x in (g, twin):
        x.schedule_tti_at(first, 0.101)   # every cell stores an image under epoch 5
    cell1 = _state(g, K)[1]
    calls = _calls(2, U, 530, epoch=6)
    nows = np.array([0.102 + 0.001 * np.arange(T), 0.1025 + 0.001 * np.arange(T)])   # a clock per cell
    rands = _pairs(rng, 2, T)
    _same_runs(g.run_at(calls, nows, rands, cell_ids=[2, 0]), _one_at_a_time(twin, calls, nows, rands, cell_ids=[2, 0]), "cell_ids [2, 0]")
    assert _state(g, K)[1] == cell1, "cell 1 was not named: averages, pending bytes, last_update, slice offsets"
    assert _state(g, K) == _state(twin, K)
    # ... and its image: the call after the run is still served from it
    reused = g.image_stats[0]
    again = [dict(first[1], rand0=21, rand1=22)]
    _same(g.schedule_tti_at(again, 0.2, cell_ids=[1])[0], twin.schedule_tti_at(again, 0.2, cell_ids=[1])[0], "cell 1 after the run")
    assert g.image_stats[0] == reused + 1 and g.image_stats == twin.image_stats
    g.close()
    twin.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. reports, 7. clock
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["epoch 0", "per-PRB under a number", "per-PRB under 0"])
def test_reports(rs, kind):
    """Without a cqi_epoch every TTI of the run reads the slot's block again and the image ends; per-PRB reports under a number are read
    from the cell's store from TTI 1 on (and from TTI 0 on in the second run, which repeats the number); under 0 from the slot each TTI."""
    sc, g, twin, rng = _pair_of_groups(rs, 9, 61)
    U, T = sc.n_users, 4
    epoch = 9 if "number" in kind else 0
    if kind == "epoch 0":
        calls = _calls(K, U, 610, epoch=0)
    else:
        calls = [dict(cqi_prb=synth_cqi(620 + k, (U, R * G), HIST), cqi_epoch=epoch) for k in range(K)]
    now = 0.1
    for run in range(2):
        nows = now + 0.001 * np.arange(1, T + 1)
        now = float(nows[-1])
        rands = _pairs(rng, K, T)
        _same_runs(g.run_at(calls, nows, rands), _one_at_a_time(twin, calls, nows, rands), f"{kind}, run {run}")
        assert _state(g, K) == _state(twin, K)
        assert g.image_stats == twin.image_stats
    assert g.image_stats == (((2 * T - 1) * K, K, 0) if epoch else (0, 0, 2 * T * K))
    g.close()
    twin.close()


def test_a_clock_that_repeats_a_value(rs):
    """now[t] == now[t-1] in the middle of a run: the reference's early return -- no update, the grants of both TTIs wait for the next."""
    sc, g, twin, rng = _pair_of_groups(rs, 9, 71)
    calls = _calls(K, sc.n_users, 710, epoch=2)
    nows = np.array([0.101, 0.102, 0.102, 0.102, 0.103, 0.103])
    rands = _pairs(rng, K, len(nows))
    _same_runs(g.run_at(calls, nows, rands), _one_at_a_time(twin, calls, nows, rands), "repeated clock")
    assert _state(g, K) == _state(twin, K)
    assert g.get_avg(0)[2] == 0.103
    g.close()
    twin.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------------------------------------------------------

def _refusals(rs, g, n_cells):
    def refused(code, frag, fn):
        before = (g.launch_count, g.image_stats, [g.slice_offset(k).tobytes() for k in range(n_cells)])
        with pytest.raises(rs.RadioSaberError) as e:
            fn()
        assert e.value.code == code and frag in str(e.value), str(e.value)
        assert (g.launch_count, g.image_stats, [g.slice_offset(k).tobytes() for k in range(n_cells)]) == before
    return refused


def test_refusals(rs):
    sc = rs.SliceConfig(UES, weight=W)
    U, T = sc.n_users, 3
    g = rs.GroupScheduler(sc, R, G, K, sched=9)
    rng = np.random.default_rng(8)
    good = rng.uniform(1e3, 5e6, U)
    for k in (0, 1):
        g.set_avg(k, good, 0.1)
    g.run_at(_calls(2, U, 800, epoch=1), 0.1 + 0.001 * np.arange(1, T + 1), _pairs(rng, 2, T))   # bytes are pending, an image is stored
    kept = [tuple(x.tobytes() if isinstance(x, np.ndarray) else x for x in g.get_avg(k)) for k in (0, 1)]
    refused = _refusals(rs, g, K)
    calls, nows, rands = _calls(2, U, 810, epoch=2), 0.2 + 0.001 * np.arange(T), _pairs(rng, 2, T)
    one = lambda **kw: [dict(c, **kw) for c in calls]   # noqa: E731
    refused(-1, "n_ttis", lambda: g.run_at(calls, np.zeros(0), np.zeros((2, 0, 2), np.int32)))
    refused(-1, "n_ttis", lambda: g.run_at(calls, 0.2 + 0.001 * np.arange(65), _pairs(rng, 2, 65)))
    refused(-1, "twice", lambda: g.run_at(calls, nows, rands, cell_ids=[1, 1]))
    refused(-1, "outside", lambda: g.run_at(calls, nows, rands, cell_ids=[0, 3]))
    refused(-1, "cqi_prb", lambda: g.run_at([calls[0], dict(cqi_prb=synth_cqi(1, (U, R * G), HIST), cqi_epoch=2)], nows, rands))
    refused(-1, "avg_rate", lambda: g.run_at(one(avg_rate=good), nows, rands))
    refused(-4, "cell 2", lambda: g.run_at(_calls(K, U, 820, epoch=2), nows, _pairs(rng, K, T)))   # RS_ERR_STATE: cell 2 is not resident
    refused(-1, "hol_delay", lambda: g.run_at(one(hol_delay=np.zeros(U)), nows, rands))
    refused(-1, "prio_has_data", lambda: g.run_at(one(prio_has_data=np.ones(U, np.uint8)), nows, rands))
    refused(-1, "required_rbs", lambda: g.run_at(one(required_rbs=np.ones(U, np.int32)), nows, rands))
    refused(-1, "data_to_transmit", lambda: g.run_at(one(data_to_transmit=np.ones(U, np.int32)), nows, rands))
    refused(-1, "rands", lambda: g.run_at(calls, nows, None))
    refused(-1, "before", lambda: g.run_at(calls, 0.05 + 0.001 * np.arange(T), rands))
    refused(-1, "not finite", lambda: g.run_at(calls, np.array([0.2, np.nan, 0.202]), rands))
    refused(-1, "neither 0 nor", lambda: g.run_at(calls, np.array([0.1 + 0.001 * T + 2.0**-30, 0.2, 0.201]), rands))   # too close to the last update
    refused(-1, "clock step", lambda: g.run_at(calls, np.array([0.2, 0.2 + 2.0**-30, 0.202]), rands))
    refused(-1, "clock step", lambda: g.run_at(calls, np.array([0.2, 0.201, 0.2005]), rands))   # backwards
    assert [tuple(x.tobytes() if isinstance(x, np.ndarray) else x for x in g.get_avg(k)) for k in (0, 1)] == kept
    # a bearer-resident cell
    g.set_bearers(2, np.ones((U, 2), np.uint8), np.full((U, 2), 1e4), 0.1)
    refused(-4, "bearer-resident", lambda: g.run_at(_calls(1, U, 830, epoch=2), nows, _pairs(rng, 1, T), cell_ids=[2]))
    g.close()


def test_refusals_of_configs_and_schedulers(rs):
    U, T = sum(UES), 3
    rng = np.random.default_rng(81)
    good = rng.uniform(1e3, 5e6, U)
    nows, rands = 0.2 + 0.001 * np.arange(T), _pairs(rng, 1, T)
    for frag, code, kw, sched, resident in (("exponents", -1, dict(algo_epsilon=[1, 2, 1], algo_psi=[1, 1, 1]), 9, "avg"),
                                            ("algo_alpha", -1, dict(algo_alpha=[1, 0, 0], algo_beta=[0, 0, 0]), 9, "avg"),
                                            ("RS_SCHED_NVS", -1, {}, 7, "avg"),
                                            ("flow-resident", -4, {}, 1, "flows")):
        sc = rs.SliceConfig(UES, weight=W, **kw)
        g = rs.GroupScheduler(sc, R, G, 1, sched=sched)
        if resident == "avg":
            g.set_avg(0, good, 0.1)
        else:
            g.set_flows(0, np.ones((U, 2), np.uint8), np.full((U, 2), 1e4), 0.1)
        _refusals(rs, g, 1)(code, frag, lambda: g.run_at(_calls(1, U, 840, epoch=1), nows, rands))
        g.close()
    # RS_SCHED_PF draws no rand(): rands may be None there, and only there
    sc = rs.SliceConfig(UES, weight=W)
    g, twin = rs.GroupScheduler(sc, R, G, 1, sched=1), rs.GroupScheduler(sc, R, G, 1, sched=1)
    for x in (g, twin):
        x.set_avg(0, good, 0.1)
    calls = _calls(1, U, 850, epoch=1)
    _same_runs(g.run_at(calls, nows, None), _one_at_a_time(twin, calls, nows, np.zeros((1, T, 2), np.int32)), "scheduler 1 without rands")
    g.close()
    twin.close()


def test_upper_lists_are_given_by_every_tti_or_by_none(rs):
    """Scheduler 10: a run whose second TTI gives no upper_* arrays -- built by hand, GroupScheduler.run_at always gives them."""
    sc = rs.SliceConfig(UES, weight=W)
    U, T = sc.n_users, 2
    g = rs.GroupScheduler(sc, R, G, 1, sched=10)
    g.set_avg(0, np.full(U, 1e4), 0.1)
    ins, outs, keep = (rs.api._TtiIn * 1)(), (rs.api._TtiOut * T)(), []
    for t in range(T):
        tin, tout, res, arrays = rs.api._marshal_tti(sc.n_slices, R, G, 10, synth_cqi(860, (U, R), HIST), None)
        keep.append((res, arrays))
        ins[0], outs[t] = tin, tout
    outs[1].upper_rbg, outs[1].upper_user = None, None
    nows, rands = np.array([0.101, 0.102]), np.zeros((1, T, 2), np.int32)
    rc = rs.lib().rs_group_run_at(g._h, 1, None, ins, T, nows.ctypes.data_as(C.POINTER(C.c_double)), rands.ctypes.data_as(C.POINTER(C.c_int32)), outs)
    assert rc == -1 and "upper_rbg" in rs.lib().rs_last_error().decode()
    assert g.launch_count == 0 and g.get_avg(0)[2] == 0.1
    g.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 9. coexistence
# ---------------------------------------------------------------------------------------------------------------------------

def _mixed_sequence(rs, g, twin, rng, U, named):
    """run, single at-call, plain schedule_tti, run -- the twin does every TTI with a call of its own."""
    now, T = 0.1, 5
    for i, step in enumerate(("run", "at", "plain", "run")):
        calls = _calls(K, U, 900 + 10 * i, epoch=1 + i // 2)
        if step == "run":
            nows = now + 0.001 * np.arange(1, T + 1)
            now = float(nows[-1])
            rands = _pairs(rng, K, T)
            _same_runs(g.run_at(calls, nows, rands), _one_at_a_time(twin, calls, nows, rands), f"step {i} ({step})")
            assert g.kernel_name == named["run"]
        elif step == "at":
            now += 0.001
            calls = [dict(c, rand0=5, rand1=6) for c in calls]
            for k, (a, b) in enumerate(zip(g.schedule_tti_at(calls, now), twin.schedule_tti_at(calls, now))):
                _same(a, b, f"step {i} ({step}) cell {k}")
            assert g.kernel_name == named["at"]
        else:
            calls = [dict(c, rand0=7, rand1=8, avg_rate=rng.uniform(1e3, 5e6, U)) for c in calls]
            for k, (a, b) in enumerate(zip(g.schedule_tti(calls), twin.schedule_tti(calls))):
                _same(a, b, f"step {i} ({step}) cell {k}")
        assert _state(g, K) == _state(twin, K), f"state after step {i} ({step})"
        assert g.image_stats == twin.image_stats


def test_coexistence_with_single_calls(rs):
    sc, g, twin, rng = _pair_of_groups(rs, 9, 91)
    name = g.kernel_name
    _mixed_sequence(rs, g, twin, rng, sc.n_users, dict(run="rs_group_run_kernel<9, 1>", at="rs_group_resident_kernel<9, 1>"))
    assert name != g.kernel_name
    g.close()
    twin.close()


def test_after_specialize_a_run_executes_the_built_in_kernel(rs):
    sc, g, twin, rng = _pair_of_groups(rs, 9, 92, jit=True, jit_resident=True)
    assert g.jit_status()[0] == 1 and g.resident_jit_status()[0] == 1
    _mixed_sequence(rs, g, twin, rng, sc.n_users, dict(run="rs_group_run_kernel<9, 1>", at="rs_group_resident_kernel_jit"))
    assert g.jit_status()[0] == 1 and g.resident_jit_status()[0] == 1
    g.close()
    twin.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 10. bounds
# ---------------------------------------------------------------------------------------------------------------------------

def test_the_longest_run(rs):
    """T = RS_GROUP_MAX_RUN on the base shape: the output blocks grow to 3 x 64 slots, and a single call afterwards still works."""
    sc, g, twin, rng = _pair_of_groups(rs, 9, 101)
    T = 64
    calls = _calls(K, sc.n_users, 1010, epoch=1)
    nows = 0.1 + 0.001 * np.arange(1, T + 1)
    rands = _pairs(rng, K, T)
    _same_runs(g.run_at(calls, nows, rands), _one_at_a_time(twin, calls, nows, rands), "T = 64")
    assert _state(g, K) == _state(twin, K)
    assert g.image_stats == twin.image_stats == (K * (T - 1), K, 0)
    again = [dict(c, rand0=1, rand1=2) for c in calls]
    for k, (a, b) in enumerate(zip(g.schedule_tti_at(again, 0.2), twin.schedule_tti_at(again, 0.2))):
        _same(a, b, f"the call after the run, cell {k}")
    g.close()
    twin.close()


def test_more_slots_than_compute_units(rs):
    """300 cells of 2 + 2 users, 4 RBGs, T = 3: several dispatch rounds of a workgroup that lives three TTIs.  The call completes, every
    (cell, TTI) has an allocation, and cells 0, 150 and 299 equal a twin's."""
    n_cells, T, probe = 300, 3, [0, 150, 299]
    sc = rs.SliceConfig([2, 2], weight=[0.5, 0.5])
    g, twin = rs.GroupScheduler(sc, 4, G, n_cells, sched=9), rs.GroupScheduler(sc, 4, G, n_cells, sched=9)
    rng = np.random.default_rng(102)
    a0 = rng.uniform(1e3, 5e6, (n_cells, sc.n_users))
    for k in range(n_cells):
        g.set_avg(k, a0[k], 0.1)
    for k in probe:
        twin.set_avg(k, a0[k], 0.1)
    calls = _calls(n_cells, sc.n_users, 1020, epoch=1, n_rbgs=4)
    nows = 0.1 + 0.001 * np.arange(1, T + 1)
    rands = _pairs(rng, n_cells, T)
    res = g.run_at(calls, nows, rands)
    assert g.launch_count == 1
    for k in range(n_cells):
        for t in range(T):
            assert (res[k][t].rbg_to_user >= 0).any() and res[k][t].user_tbs_bits.any(), f"cell {k} TTI {t}: nothing was written"
    ref = _one_at_a_time(twin, [calls[k] for k in probe], nows, rands[probe], cell_ids=probe)
    _same_runs([res[k] for k in probe], ref, "300 cells")
    for k in probe:
        a, pend, last = g.get_avg(k)
        b, pend2, last2 = twin.get_avg(k)
        assert (a.tobytes(), pend.tobytes(), last, g.slice_offset(k).tobytes()) == (b.tobytes(), pend2.tobytes(), last2, twin.slice_offset(k).tobytes())
    g.close()
    twin.close()
