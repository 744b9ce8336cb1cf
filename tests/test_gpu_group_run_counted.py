"""rs_group_run_counted_at / GroupScheduler.run_counted_at: rs_group_run_at with per-user byte and RB counters on the device, with or
without per-TTI outputs.  A counted run is defined as a run plus a credit, so the expectation is a twin group fed by run_at -- its
outputs say what every grant was --, and the oracle's own DoStopSchedule counters where the oracle restates the scheduler.  Every
comparison is bitwise.  The twin's side and the counted side of the base case are computed once per (scheduler, T) and shared."""
import functools

import numpy as np
import pytest

from conftest import synth_cqi
from test_gpu_group import HIST, _same
from test_gpu_group_run import G, K, R, RUN_SCHEDS, UES, W, _calls, _pairs, _refusals, _same_runs, _state

pytestmark = pytest.mark.gpu

N_RUNS = 3


def _start(seed, n_cells, U):
    """Non-zero counters to start from, per cell: above 2^32, so that a 32-bit add would show."""
    rng = np.random.default_rng(seed)
    return [(rng.integers(1, 2**40, U), rng.integers(1, 2**34, U)) for _ in range(n_cells)]


def _grants(res, U, ids=None):
    """What DoStopSchedule credits for one cell's run, from its outputs: per user id the sums over the TTIs of min(tbs_bits // 8, 1e8) and
    of the PRBs of the positions that were granted bytes."""
    cb, cr = np.zeros(U, np.int64), np.zeros(U, np.int64)
    ids = np.arange(len(res[0].user_tbs_bits)) if ids is None else np.asarray(ids)
    for out in res:
        bytes_ = np.minimum(out.user_tbs_bits.astype(np.int64) // 8, 100000000)
        cb[ids] += bytes_
        cr[ids] += np.where(bytes_ != 0, out.user_nprb.astype(np.int64), 0)
    return cb, cr


def _counters(g, n_cells):
    return [tuple(x.copy() for x in g.get_avg_counters(k)) for k in range(n_cells)]


def _same_counters(got, want, what):
    for k, ((cb, cr), (wb, wr)) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(cb, wb, err_msg=f"{what}: cell {k}, cum_bytes")
        np.testing.assert_array_equal(cr, wr, err_msg=f"{what}: cell {k}, cum_rbs")


def _inputs(sched, T, ues=tuple(UES), n_rbgs=R, n_cells=K):
    """The base case's inputs: starting averages and, per run, new grids under a new cqi_epoch, the clock and the rand() pairs."""
    U = sum(ues)
    rng = np.random.default_rng(100 * sched + T)
    a0 = [rng.uniform(1e3, 5e6, U) for _ in range(n_cells)]
    runs, now = [], 0.1
    for run in range(N_RUNS):
        nows = now + 0.001 * np.arange(1, T + 1)
        now = float(nows[-1])
        runs.append(dict(calls=_calls(n_cells, U, 1000 * sched + 10 * run + T, epoch=1 + run, n_rbgs=n_rbgs), nows=nows, rands=_pairs(rng, n_cells, T)))
    return a0, runs


def _record(g, n_cells, counted):
    return dict(state=_state(g, n_cells), stats=g.image_stats, launches=g.launch_count, counters=_counters(g, n_cells) if counted else None,
                name=g.kernel_name)


@functools.lru_cache(maxsize=None)
def _base_case(sched, T, side):
    """One side of the base case, run once and shared by the tests below: `twin` is fed by run_at, `counted` by run_counted_at,
    `silent` by run_counted_at(outputs=False).  Per run: the outputs (None for `silent`) and what the group holds afterwards."""
    import radiosaber_amd as rs
    a0, runs = _inputs(sched, T)
    sc = rs.SliceConfig(UES, weight=W)
    g = rs.GroupScheduler(sc, R, G, K, sched=sched)
    start = _start(7 * sched + T, K, sc.n_users)
    for k in range(K):
        g.set_avg(k, a0[k], 0.1)
        if side != "twin":
            g.set_avg_counters(k, *start[k])
    out = []
    for run in runs:
        if side == "twin":
            res = g.run_at(run["calls"], run["nows"], run["rands"])
        else:
            res = g.run_counted_at(run["calls"], run["nows"], run["rands"], outputs=side == "counted")
        out.append(dict(res=res, **_record(g, K, side != "twin")))
    g.close()
    return start, out


@functools.lru_cache(maxsize=None)
def _oracle_counters(sched, T):
    """The oracle's m_cumulateBytes / m_cumulateRBs behind each run of the base case (rso_cell_step's DoStopSchedule), from zero."""
    from oracle import oracle_py as oracle
    a0, runs = _inputs(sched, T)
    cells = [oracle.Cell(list(UES), R, G, sched, weights=list(W)) for _ in range(K)]
    for k in range(K):
        cells[k].set_avg_rate(a0[k])
        cells[k].set_last_update(0.1)
    after = []
    for run in runs:
        for k in range(K):
            cells[k].set_cqi(run["calls"][k]["cqi"])
            for t in range(T):
                assert cells[k].step(float(run["nows"][t]), int(run["rands"][k, t, 0]), int(run["rands"][k, t, 1]), cells[k].new_out()) == 0
        after.append([(cells[k].state()["cum_bytes"].copy(), cells[k].state()["cum_rbs"].copy()) for k in range(K)])
    return after


CASES = [(sched, T) for sched in RUN_SCHEDS for T in (1, 2, 7)]


# ---------------------------------------------------------------------------------------------------------------------------
# 1. a counted run is a run
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sched,T", CASES)
def test_a_counted_run_is_a_run(rs, sched, T):
    """Three runs in a row, new grids and a new cqi_epoch before each: every output field of every (cell, TTI) -- scheduler 10 with its
    upper_* lists --, after each run the averages, pending bytes, last_update, slice offsets and image_stats; 3 launches each."""
    _, twin = _base_case(sched, T, "twin")
    _, got = _base_case(sched, T, "counted")
    for i, (a, b) in enumerate(zip(got, twin)):
        _same_runs(a["res"], b["res"], f"sched {sched} T {T} run {i}", upper=sched == 10)
        assert a["state"] == b["state"], f"sched {sched} T {T}: state after run {i}"
        assert a["stats"] == b["stats"] == ((i + 1) * K * (T - 1), (i + 1) * K, 0)
        assert a["name"].startswith(f"rs_group_run_counted_kernel<{sched}, ") and b["name"].startswith(f"rs_group_run_kernel<{sched}, ")
    assert (got[-1]["launches"], twin[-1]["launches"]) == (3, 3)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the counters are the sum of the grants
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sched,T", CASES)
def test_the_counters_are_the_sum_of_the_grants(rs, oracle, sched, T):
    """From non-zero counters: after each run they are the start values plus, per user id, the twin's min(user_tbs_bits // 8, 1e8) and
    user_nprb summed over TTIs and positions -- and the start values plus the oracle's own counters."""
    U = sum(UES)
    start, got = _base_case(sched, T, "counted")
    _, twin = _base_case(sched, T, "twin")
    ref = _oracle_counters(sched, T)
    want = [(b.copy(), r.copy()) for b, r in start]
    moved = False
    for i in range(N_RUNS):
        for k in range(K):
            cb, cr = _grants(twin[i]["res"][k], U)
            moved |= bool(cb.any() and cr.any())
            want[k][0][:] += cb
            want[k][1][:] += cr
        _same_counters(got[i]["counters"], want, f"sched {sched} T {T} after run {i}")
        _same_counters(got[i]["counters"], [(start[k][0] + ref[i][k][0], start[k][1] + ref[i][k][1]) for k in range(K)],
                       f"sched {sched} T {T} after run {i}, against the oracle")
    assert moved, "not vacuous: grants were made"


# ---------------------------------------------------------------------------------------------------------------------------
# 3. without outputs
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sched,T", CASES)
def test_without_outputs(rs, sched, T):
    """The same three runs with outputs=False: nothing comes back, and state, counters and image_stats after each run are the twin's and
    the counted side's; 3 launches."""
    _, twin = _base_case(sched, T, "twin")
    _, counted = _base_case(sched, T, "counted")
    start, got = _base_case(sched, T, "silent")
    for i in range(N_RUNS):
        assert got[i]["res"] is None
        assert got[i]["state"] == twin[i]["state"], f"sched {sched} T {T}: state after run {i}"
        assert got[i]["stats"] == twin[i]["stats"]
        _same_counters(got[i]["counters"], counted[i]["counters"], f"sched {sched} T {T} after run {i}, no outputs")
        assert got[i]["name"] == counted[i]["name"]
    assert got[-1]["launches"] == 3
    assert any((got[-1]["counters"][k][0] != start[k][0]).any() for k in range(K))


def test_without_outputs_the_output_blocks_do_not_grow(rs):
    """A first run of T = 7 without outputs, then the same group serves a run with outputs and a single at-call: the output blocks were
    left as they were (K slots) by the first and grow with the second; all three agree with a twin."""
    sched, T = 9, 7
    a0, runs = _inputs(sched, T)
    sc = rs.SliceConfig(UES, weight=W)
    g, twin = rs.GroupScheduler(sc, R, G, K, sched=sched), rs.GroupScheduler(sc, R, G, K, sched=sched)
    for k in range(K):
        g.set_avg(k, a0[k], 0.1)
        twin.set_avg(k, a0[k], 0.1)
        g.set_avg_counters(k)
    assert g.run_counted_at(runs[0]["calls"], runs[0]["nows"], runs[0]["rands"], outputs=False) is None
    twin.run_at(runs[0]["calls"], runs[0]["nows"], runs[0]["rands"])
    assert _state(g, K) == _state(twin, K)
    _same_runs(g.run_counted_at(runs[1]["calls"], runs[1]["nows"], runs[1]["rands"]), twin.run_at(runs[1]["calls"], runs[1]["nows"], runs[1]["rands"]),
               "the run with outputs behind the run without")
    again = [dict(c, rand0=1, rand1=2) for c in runs[1]["calls"]]
    for k, (a, b) in enumerate(zip(g.schedule_tti_at(again, 0.2), twin.schedule_tti_at(again, 0.2))):
        _same(a, b, f"the call after the runs, cell {k}")
    assert _state(g, K) == _state(twin, K) and g.image_stats == twin.image_stats
    g.close()
    twin.close()


@pytest.mark.parametrize("outputs", [True, False])
def test_per_prb_reports(rs, outputs):
    """Per-PRB reports under a number: the group copies its blocks instead of sharing them with the device, and from TTI 1 on the link
    adaptation reads the cell's store.  Two runs (the second repeats the number: TTI 0 reads the store too), with and without outputs:
    results, state, image_stats and counters against a twin's run_at."""
    sched, T = 9, 3
    sc = rs.SliceConfig(UES, weight=W)
    U = sc.n_users
    g, twin = rs.GroupScheduler(sc, R, G, K, sched=sched), rs.GroupScheduler(sc, R, G, K, sched=sched)
    rng = np.random.default_rng(31)
    for k in range(K):
        a0 = rng.uniform(1e3, 5e6, U)
        g.set_avg(k, a0, 0.1)
        twin.set_avg(k, a0, 0.1)
        g.set_avg_counters(k)
    calls = [dict(cqi_prb=synth_cqi(310 + k, (U, R * G), HIST), cqi_epoch=4) for k in range(K)]
    want = [(np.zeros(U, np.int64), np.zeros(U, np.int64)) for _ in range(K)]
    now = 0.1
    for run in range(2):
        nows = now + 0.001 * np.arange(1, T + 1)
        now = float(nows[-1])
        rands = _pairs(rng, K, T)
        ref = twin.run_at(calls, nows, rands)
        res = g.run_counted_at(calls, nows, rands, outputs=outputs)
        if outputs:
            _same_runs(res, ref, f"per-PRB reports, run {run}")
        else:
            assert res is None
        for k in range(K):
            cb, cr = _grants(ref[k], U)
            want[k][0][:] += cb
            want[k][1][:] += cr
        assert _state(g, K) == _state(twin, K) and g.image_stats == twin.image_stats
        _same_counters(_counters(g, K), want, f"per-PRB reports, run {run}")
    assert g.image_stats == ((2 * T - 1) * K, K, 0)
    g.close()
    twin.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. by user id
# ---------------------------------------------------------------------------------------------------------------------------

def test_by_user_id(rs):
    """A call names a strict subset of the users through user_id, so that call position i is user ids[i] != i (a run's users ascend, as
    every drop-in call's: a list that does not is refused), two runs: the named users' counters move by their grants, every other
    user's are bit for bit the start values."""
    sched, T = 9, 3
    sc = rs.SliceConfig(UES, weight=W)
    U = sc.n_users
    ids = np.array([1, 2, 4, 6, 7, 10, 11], np.int32)
    others = np.setdiff1d(np.arange(U), ids)
    g, twin = rs.GroupScheduler(sc, R, G, K, sched=sched), rs.GroupScheduler(sc, R, G, K, sched=sched)
    rng = np.random.default_rng(41)
    start = _start(42, K, U)
    for k in range(K):
        a0 = rng.uniform(1e3, 5e6, U)
        g.set_avg(k, a0, 0.1)
        twin.set_avg(k, a0, 0.1)
        g.set_avg_counters(k, *start[k])
    want = [(b.copy(), r.copy()) for b, r in start]
    now = 0.1
    for run in range(2):
        calls = [dict(cqi=synth_cqi(410 + 10 * run + k, (len(ids), R), HIST), user_id=ids, cqi_epoch=1 + run) for k in range(K)]
        nows = now + 0.001 * np.arange(1, T + 1)
        now = float(nows[-1])
        rands = _pairs(rng, K, T)
        ref = twin.run_at(calls, nows, rands)
        _same_runs(g.run_counted_at(calls, nows, rands), ref, f"7 of 12 users, run {run}")
        for k in range(K):
            cb, cr = _grants(ref[k], U, ids)
            assert cb[ids].any() and not cb[others].any()
            want[k][0][:] += cb
            want[k][1][:] += cr
        got = _counters(g, K)
        _same_counters(got, want, f"run {run}")
        for k in range(K):
            assert got[k][0][others].tobytes() == start[k][0][others].tobytes() and got[k][1][others].tobytes() == start[k][1][others].tobytes()
        assert _state(g, K) == _state(twin, K)
    before = _counters(g, K)
    permuted = [dict(c, user_id=ids[::-1].copy()) for c in calls]
    _refusals(rs, g, K)(-1, "ascend", lambda: g.run_counted_at(permuted, now + 0.001 * np.arange(1, T + 1), _pairs(rng, K, T)))
    _same_counters(_counters(g, K), before, "a refused user list")
    g.close()
    twin.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. mask words
# ---------------------------------------------------------------------------------------------------------------------------

MASK_SHAPES = {"70 users": dict(ues=(30, 25, 15), w=(0.4, 0.35, 0.25), n_rbgs=8, g_size=2, seed=5100),
               "64 RBGs": dict(ues=(3,), w=(1.0,), n_rbgs=64, g_size=1, seed=5200)}


def _mask_inputs(ues, w, n_rbgs, g_size, seed):
    U, T = sum(ues), 2
    rng = np.random.default_rng(seed)
    return dict(a0=rng.uniform(1e3, 5e6, U), cqi=synth_cqi(seed + 1, (U, n_rbgs), HIST), nows=np.array([0.101, 0.102]), rands=_pairs(rng, 1, T))


@pytest.mark.parametrize("shape", list(MASK_SHAPES))
def test_the_mask_words_case_is_not_vacuous(oracle, shape):
    """On the oracle's side (no GPU needed for the answer): with 70 users a user at call position >= 63 -- owner + 1 >= 64, the second
    entry of maskB -- is served in some TTI; with 64 RBGs some user holds RBG 63, lane 63."""
    s = MASK_SHAPES[shape]
    x = _mask_inputs(s["ues"], s["w"], s["n_rbgs"], s["g_size"], s["seed"])
    cell = oracle.Cell(list(s["ues"]), s["n_rbgs"], s["g_size"], 9, weights=list(s["w"]))
    cell.set_avg_rate(x["a0"])
    cell.set_last_update(0.1)
    cell.set_cqi(x["cqi"])
    high, last_lane = False, False
    for t in range(2):
        out = cell.new_out()
        assert cell.step(float(x["nows"][t]), int(x["rands"][0, t, 0]), int(x["rands"][0, t, 1]), out) == 0
        high |= bool((out.user_tbs_bits[64:] > 0).any()) if sum(s["ues"]) > 64 else False
        last_lane |= s["n_rbgs"] == 64 and out.rbg_to_user[63] >= 0
    assert high if shape == "70 users" else last_lane


@pytest.mark.parametrize("shape", list(MASK_SHAPES))
def test_mask_words(rs, shape):
    """One cell of 70 users in slices of 30 / 25 / 15 with 8 RBGs (positions >= 63 lie in maskB's second entry), and one of 3 users in one
    slice with 64 RBGs of 1 PRB (lane 63): scheduler 9, T = 2, the counters against the twin's grants."""
    s = MASK_SHAPES[shape]
    x = _mask_inputs(s["ues"], s["w"], s["n_rbgs"], s["g_size"], s["seed"])
    sc = rs.SliceConfig(list(s["ues"]), weight=list(s["w"]))
    U = sc.n_users
    g, twin = rs.GroupScheduler(sc, s["n_rbgs"], s["g_size"], 1, sched=9), rs.GroupScheduler(sc, s["n_rbgs"], s["g_size"], 1, sched=9)
    start = _start(s["seed"], 1, U)
    g.set_avg(0, x["a0"], 0.1)
    twin.set_avg(0, x["a0"], 0.1)
    g.set_avg_counters(0, *start[0])
    calls = [dict(cqi=x["cqi"], cqi_epoch=1)]
    ref = twin.run_at(calls, x["nows"], x["rands"])
    _same_runs(g.run_counted_at(calls, x["nows"], x["rands"]), ref, shape)
    cb, cr = _grants(ref[0], U)
    if shape == "70 users":
        assert cb[64:].any(), "a user at position >= 64 was served"
    else:
        assert any(out.rbg_to_user[63] >= 0 for out in ref[0]), "some user holds RBG 63"
    _same_counters(_counters(g, 1), [(start[0][0] + cb, start[0][1] + cr)], shape)
    assert cr.sum() == sum(int(np.where(out.user_tbs_bits // 8 != 0, out.user_nprb, 0).sum()) for out in ref[0])
    g.close()
    twin.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. a zero clock step
# ---------------------------------------------------------------------------------------------------------------------------

def test_a_zero_clock_step_still_credits(rs):
    """now[k][1] == now[k][0]: TTI 1 updates nothing -- the averages are those of the one-TTI run -- and still credits its grants."""
    sched = 9
    a0, runs = _inputs(sched, 2)
    sc = rs.SliceConfig(UES, weight=W)
    U = sc.n_users
    g, one, twin = (rs.GroupScheduler(sc, R, G, K, sched=sched) for _ in range(3))
    for k in range(K):
        for x in (g, one, twin):
            x.set_avg(k, a0[k], 0.1)
        g.set_avg_counters(k)
        one.set_avg_counters(k)
    calls, rands = runs[0]["calls"], runs[0]["rands"]
    nows = np.array([0.101, 0.101])
    ref = twin.run_at(calls, nows, rands)
    _same_runs(g.run_counted_at(calls, nows, rands), ref, "a repeated clock value")
    one.run_counted_at(calls, nows[:1], rands[:, :1])
    assert _state(g, K) == _state(twin, K)
    for k in range(K):
        assert g.get_avg(k)[0].tobytes() == one.get_avg(k)[0].tobytes(), "the averages did not move in TTI 1"
        both, first = _grants(ref[k], U), _grants(ref[k][:1], U)
        second = _grants(ref[k][1:], U)
        assert second[0].any() and second[1].any()
        _same_counters([g.get_avg_counters(k)], [both], f"cell {k}: both TTIs are credited")
        _same_counters([one.get_avg_counters(k)], [first], f"cell {k}: the one-TTI run")
    for x in (g, one, twin):
        x.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 7. rules
# ---------------------------------------------------------------------------------------------------------------------------

def test_rules(rs):
    sc = rs.SliceConfig(UES, weight=W)
    U, T = sc.n_users, 3
    g = rs.GroupScheduler(sc, R, G, K, sched=9)
    rng = np.random.default_rng(70)
    good = rng.uniform(1e3, 5e6, U)
    start = _start(71, K, U)
    refused = _refusals(rs, g, K)
    # not average-resident: RS_ERR_STATE, the message names the cell; and nobody is avg-counted yet
    refused(-4, "cell 1", lambda: g.set_avg_counters(1, *start[1]))
    for k in range(K):
        g.set_avg(k, good, 0.1)
    refused(-4, "cell 2", lambda: g.get_avg_counters(2))
    refused(-1, "negative", lambda: g.set_avg_counters(0, np.full(U, -1, np.int64), None))
    refused(-1, "negative", lambda: g.set_avg_counters(0, None, np.where(np.arange(U) == 3, -5, 0).astype(np.int64)))
    refused(-4, "cell 0", lambda: g.get_avg_counters(0))   # (a refused set leaves the cell as it was)
    for k in (0, 1):
        g.set_avg_counters(k, *start[k])
    calls, nows, rands = _calls(K, U, 700, epoch=1), 0.1 + 0.001 * np.arange(1, T + 1), _pairs(rng, K, T)
    # average-resident but not avg-counted
    refused(-4, "cell 2 is not avg-counted", lambda: g.run_counted_at(calls, nows, rands))
    refused(-4, "cell 2 is not avg-counted", lambda: g.run_counted_at(calls, nows, rands, outputs=False))
    two = calls[:2]
    # a rejected call moves no counter and launches nothing (refused() checks the launch count, image_stats and slice offsets)
    for outputs in (True, False):
        refused(-1, "n_ttis", lambda: g.run_counted_at(two, np.zeros(0), np.zeros((2, 0, 2), np.int32), outputs=outputs))
        refused(-1, "n_ttis", lambda: g.run_counted_at(two, 0.2 + 0.001 * np.arange(65), _pairs(rng, 2, 65), outputs=outputs))
        refused(-1, "rands", lambda: g.run_counted_at(two, nows, None, outputs=outputs))
    _same_counters(_counters(g, 2), start[:2], "after the refusals")
    assert g.get_avg(0)[2] == 0.1
    g7 = rs.GroupScheduler(sc, R, G, 1, sched=7)
    g7.set_avg(0, good, 0.1)
    g7.set_avg_counters(0, *start[0])
    _refusals(rs, g7, 1)(-1, "RS_SCHED_NVS", lambda: g7.run_counted_at(_calls(1, U, 701, epoch=1), nows, _pairs(rng, 1, T)))
    _same_counters(_counters(g7, 1), start[:1], "scheduler 7")
    g7.close()
    # a counted run moves them; run_at, schedule_tti_at and schedule_tti on an avg-counted cell leave them alone
    g.run_counted_at(two, nows, rands[:2])
    moved = _counters(g, 2)
    assert all((moved[k][0] != start[k][0]).any() and (moved[k][1] != start[k][1]).any() for k in (0, 1))
    g.run_at(two, 0.11 + 0.001 * np.arange(T), rands[:2])
    assert g.kernel_name == "rs_group_run_kernel<9, 1>"
    g.schedule_tti_at([dict(c, rand0=3, rand1=4) for c in two], 0.12)
    g.schedule_tti([dict(c, rand0=3, rand1=4, avg_rate=good) for c in two])
    _same_counters(_counters(g, 2), moved, "calls that do not count")
    # rs_group_get_counters / rs_group_set_counters stay bearer-only
    refused(-4, "cell 0 is not counted", lambda: g.get_counters(0))
    refused(-4, "cell 0 is not bearer-resident", lambda: g.set_counters(0))
    # rs_group_set_avg keeps the state and the counters
    g.set_avg(0, good, 0.2)
    _same_counters([g.get_avg_counters(0)], moved[:1], "behind rs_group_set_avg")
    g.run_counted_at(two[:1], 0.2 + 0.001 * np.arange(1, T + 1), rands[:1])
    assert (g.get_avg_counters(0)[0] != moved[0][0]).any()
    # rs_group_set_bearers ends it
    g.set_bearers(1, np.ones((U, 2), np.uint8), np.full((U, 2), 1e4), 0.3)
    refused(-4, "cell 1", lambda: g.get_avg_counters(1))
    g.set_avg(1, good, 0.3)
    refused(-4, "cell 1 is not avg-counted", lambda: g.run_counted_at(two[:1], 0.3 + 0.001 * np.arange(1, T + 1), rands[:1], cell_ids=[1]))
    g.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 8. other forms untouched
# ---------------------------------------------------------------------------------------------------------------------------

def test_after_specialize_run_a_counted_run_executes_the_built_in_kernel(rs):
    """rs_group_specialize_run serves run_at with the group's own build and does not reach counted runs: they name the built-in kernel
    and give the results, state and counters of a group that never specialised."""
    sched, T = 9, 4
    a0, runs = _inputs(sched, T)
    sc = rs.SliceConfig(UES, weight=W)
    g, plain = rs.GroupScheduler(sc, R, G, K, sched=sched, jit_run=True), rs.GroupScheduler(sc, R, G, K, sched=sched)
    assert g.run_jit_status()[0] == 1
    for k in range(K):
        for x in (g, plain):
            x.set_avg(k, a0[k], 0.1)
            x.set_avg_counters(k)
    for i, run in enumerate(runs[:2]):
        res = g.run_counted_at(run["calls"], run["nows"], run["rands"])
        assert g.kernel_name == "rs_group_run_counted_kernel<9, 1>"
        _same_runs(res, plain.run_counted_at(run["calls"], run["nows"], run["rands"]), f"run {i}")
        assert _state(g, K) == _state(plain, K)
        _same_counters(_counters(g, K), _counters(plain, K), f"run {i}")
    run = runs[2]
    _same_runs(g.run_at(run["calls"], run["nows"], run["rands"]), plain.run_at(run["calls"], run["nows"], run["rands"]), "a plain run behind them")
    assert g.kernel_name == "rs_group_run_kernel_jit" and g.run_jit_status()[0] == 1
    assert g.run_counted_at(run["calls"], 0.2 + 0.001 * np.arange(T), run["rands"], outputs=False) is None
    assert g.kernel_name == "rs_group_run_counted_kernel<9, 1>"
    g.close()
    plain.close()
