"""rs_group_run_records_at / GroupScheduler.run_counted_at(records=True): the counted run with one grant record per credited position and
TTI, with or without per-TTI outputs.  The call is defined as rs_group_run_counted_at plus records, so the expectation is the twin group
fed by run_at -- its outputs say what every grant was -- and the counted sides of tests/test_gpu_group_run_counted.py's base case.
Every comparison is bitwise.  The sides are computed once per (scheduler, T) and shared."""
import functools

import numpy as np
import pytest

from conftest import synth_cqi
from radiosaber_amd import logfmt
from test_gpu_group import HIST
from test_gpu_group_run import G, K, R, UES, W, _calls, _pairs, _refusals, _same_runs, _state
from test_gpu_group_run_counted import (CASES, N_RUNS, _base_case, _counters, _inputs, _oracle_counters, _record, _same_counters,
                                        _start)

pytestmark = pytest.mark.gpu

FIELDS = ("pos", "user_id", "bytes", "nprb", "cum_bytes", "cum_rbs")
WG = 512   # threads of a group's workgroup: the default, and the most the kernels built into the library take


def _bytes_of(out):
    return np.minimum(out.user_tbs_bits.astype(np.int64) // 8, 100000000)


def _expected(res, start_b, start_r, ids=None):
    """The records of ONE cell's run from the twin's outputs res[t]: per TTI an array over the positions with bytes != 0, ascending; the
    running counters start at start_b / start_r (by user id, updated in place)."""
    import radiosaber_amd as rs
    want = []
    for out in res:
        b = _bytes_of(out)
        pos = np.flatnonzero(b != 0)
        uid = pos if ids is None else np.asarray(ids)[pos]
        rec = np.zeros(len(pos), rs.api.GRANT_RECORD)
        rec["pos"], rec["user_id"], rec["bytes"], rec["nprb"] = pos, uid, b[pos], out.user_nprb[pos]
        start_b[uid] += b[pos]          # (a user is named once per call: no index repeats)
        start_r[uid] += out.user_nprb[pos]
        rec["cum_bytes"], rec["cum_rbs"] = start_b[uid], start_r[uid]
        want.append(rec)
    return want


def _same_records(got, want, what):
    assert len(got) == len(want)
    for t, (a, b) in enumerate(zip(got, want)):
        assert len(a) == len(b), f"{what}, TTI {t}: {len(a)} records, the twin's outputs have {len(b)} grants"
        assert (np.diff(a["pos"]) > 0).all(), f"{what}, TTI {t}: positions do not ascend strictly"
        for f in FIELDS:
            np.testing.assert_array_equal(a[f], b[f], err_msg=f"{what}, TTI {t}: {f}")


@functools.lru_cache(maxsize=None)
def _records_case(sched, T, outputs):
    """The base case of the counted file with records on, with or without outputs: per run the outputs, the records and what the group
    holds afterwards."""
    import radiosaber_amd as rs
    a0, runs = _inputs(sched, T)
    sc = rs.SliceConfig(UES, weight=W)
    g = rs.GroupScheduler(sc, R, G, K, sched=sched)
    start = _start(7 * sched + T, K, sc.n_users)
    for k in range(K):
        g.set_avg(k, a0[k], 0.1)
        g.set_avg_counters(k, *start[k])
    bound, out = g.grant_bound, []
    for run in runs:
        res, recs = g.run_counted_at(run["calls"], run["nows"], run["rands"], outputs=outputs, records=True)
        out.append(dict(res=res, recs=recs, **_record(g, K, True)))
    g.close()
    return start, bound, out


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the records are the twin's grants, and the run is the counted run
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("outputs", [True, False], ids=["outputs", "silent"])
@pytest.mark.parametrize("sched,T", CASES)
def test_records_of_a_counted_run(rs, sched, T, outputs):
    """Three runs in a row from counters above 2^32: per (cell, TTI) as many records as the twin's outputs have positions with bytes != 0,
    ascending strictly in pos; user_id, bytes and nprb the twin's; the counters the start values plus the running sums; every user's
    last record what get_avg_counters says; and outputs, state, counters, image_stats, launch count and kernel name those of the
    counted run without records, run for run."""
    _, twin = _base_case(sched, T, "twin")
    _, base = _base_case(sched, T, "counted" if outputs else "silent")
    start, bound, got = _records_case(sched, T, outputs)
    run_b, run_r = [b.copy() for b, _ in start], [r.copy() for _, r in start]
    last = [({}, {}) for _ in range(K)]
    most = 0
    for i in range(N_RUNS):
        for k in range(K):
            want = _expected(twin[i]["res"][k], run_b[k], run_r[k])
            _same_records(got[i]["recs"][k], want, f"sched {sched} T {T} run {i} cell {k}")
            for rec in got[i]["recs"][k]:
                most = max(most, len(rec))
                for r in rec:
                    last[k][0][int(r["user_id"])], last[k][1][int(r["user_id"])] = int(r["cum_bytes"]), int(r["cum_rbs"])
        if outputs:
            _same_runs(got[i]["res"], base[i]["res"], f"sched {sched} T {T} run {i}", upper=sched == 10)
        else:
            assert got[i]["res"] is None
        assert got[i]["state"] == base[i]["state"] == twin[i]["state"], f"sched {sched} T {T}: state after run {i}"
        assert got[i]["stats"] == base[i]["stats"] and got[i]["launches"] == base[i]["launches"] == i + 1
        assert got[i]["name"] == base[i]["name"] and got[i]["name"].startswith(f"rs_group_run_counted_kernel<{sched}, ")
        _same_counters(got[i]["counters"], base[i]["counters"], f"sched {sched} T {T} after run {i}")
    for k in range(K):
        cb, cr = got[-1]["counters"][k]
        assert last[k][0], "not vacuous: the cell had grants"
        for u, v in last[k][0].items():
            assert cb[u] == v and cr[u] == last[k][1][u], f"cell {k}, user {u}: the last record against get_avg_counters"
        others = np.setdiff1d(np.arange(len(cb)), list(last[k][0]))
        assert (cb[others] == start[k][0][others]).all() and (cr[others] == start[k][1][others]).all()
    # the bound: min(U, R) where an RBG has one owner; for UpperBound no smaller than the largest count seen
    U = sum(UES)
    assert 0 < most <= bound <= U
    if sched != 10:
        assert bound == min(U, R)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. more than one wave, more than one pass, two users on one RBG
# ---------------------------------------------------------------------------------------------------------------------------

WIDE = dict(ues=(350, 350), w=(0.5, 0.5), n_rbgs=4, g_size=2, T=4)   # 700 users: positions beyond the workgroup's 512 threads


def _wide_inputs(sched):
    U, T = sum(WIDE["ues"]), WIDE["T"]
    rng = np.random.default_rng(6100 + sched)
    return dict(a0=rng.uniform(1e3, 5e6, U), cqi=synth_cqi(6200 + sched, (U, WIDE["n_rbgs"]), HIST), nows=0.1 + 0.001 * np.arange(1, T + 1),
                rands=_pairs(rng, 1, T))


def _waves(res):
    """From one cell's outputs: (a TTI has grants in two different waves, some grant at pos >= 64, some grant beyond the first pass,
    some TTI counts an RBG for two users)."""
    two, high, beyond, shared = False, False, False, False
    for out in res:
        pos = np.flatnonzero(_bytes_of(out) != 0)
        two |= len(set((pos % WG) // 64)) > 1
        high |= bool((pos >= 64).any())
        beyond |= bool((pos >= WG).any())
        shared |= int(out.user_nprb[pos].sum()) > WIDE["g_size"] * int((out.rbg_to_user >= 0).sum())
    return two, high, beyond, shared


@pytest.mark.parametrize("sched", [9, 10])
def test_the_wide_case_is_not_vacuous(oracle, sched):
    """On the oracle's side (no GPU needed for the answer): 700 users on 4 RBGs have, within four TTIs, a TTI with grants in two
    waves, a grant at a position >= 64 and one at a position >= 512 -- the second pass of a 512-thread workgroup --; scheduler 10 also
    a TTI whose PRB counts add up to more than the RBGs given out: one RBG, two users."""
    x = _wide_inputs(sched)
    cell = oracle.Cell(list(WIDE["ues"]), WIDE["n_rbgs"], WIDE["g_size"], sched, weights=list(WIDE["w"]))
    cell.set_avg_rate(x["a0"])
    cell.set_last_update(0.1)
    cell.set_cqi(x["cqi"])
    res = []
    for t in range(WIDE["T"]):
        out = cell.new_out()
        assert cell.step(float(x["nows"][t]), int(x["rands"][0, t, 0]), int(x["rands"][0, t, 1]), out) == 0
        res.append(out)
    two, high, beyond, shared = _waves(res)
    assert two and high and beyond and (shared or sched != 10)


@pytest.mark.parametrize("sched", [9, 10])
def test_records_from_several_waves_and_passes(rs, sched):
    """The wide case on the device, without outputs: the records against the twin's outputs, which show the same three properties."""
    x = _wide_inputs(sched)
    sc = rs.SliceConfig(list(WIDE["ues"]), weight=list(WIDE["w"]))
    U = sc.n_users
    g, twin = (rs.GroupScheduler(sc, WIDE["n_rbgs"], WIDE["g_size"], 1, sched=sched) for _ in range(2))
    start = _start(6300 + sched, 1, U)
    g.set_avg(0, x["a0"], 0.1)
    twin.set_avg(0, x["a0"], 0.1)
    g.set_avg_counters(0, *start[0])
    calls = [dict(cqi=x["cqi"], cqi_epoch=1)]
    ref = twin.run_at(calls, x["nows"], x["rands"])
    two, high, beyond, shared = _waves(ref[0])
    assert two and high and beyond and (shared or sched != 10)
    res, recs = g.run_counted_at(calls, x["nows"], x["rands"], outputs=False, records=True)
    assert res is None
    cb, cr = start[0][0].copy(), start[0][1].copy()
    _same_records(recs[0], _expected(ref[0], cb, cr), f"700 users, sched {sched}")
    _same_counters(_counters(g, 1), [(cb, cr)], f"700 users, sched {sched}")
    assert _state(g, 1) == _state(twin, 1)
    most = max(len(r) for r in recs[0])
    assert 0 < most <= g.grant_bound <= U
    if sched != 10:
        assert g.grant_bound == WIDE["n_rbgs"]
    g.close()
    twin.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the rest of the counted file's ground, records on
# ---------------------------------------------------------------------------------------------------------------------------

def _pair(rs, sched, seed, start_seed):
    sc = rs.SliceConfig(UES, weight=W)
    g, twin = rs.GroupScheduler(sc, R, G, K, sched=sched), rs.GroupScheduler(sc, R, G, K, sched=sched)
    rng = np.random.default_rng(seed)
    start = _start(start_seed, K, sc.n_users)
    for k in range(K):
        a0 = rng.uniform(1e3, 5e6, sc.n_users)
        g.set_avg(k, a0, 0.1)
        twin.set_avg(k, a0, 0.1)
        g.set_avg_counters(k, *start[k])
    return sc, g, twin, rng, [b.copy() for b, _ in start], [r.copy() for _, r in start]


@pytest.mark.parametrize("outputs", [True, False], ids=["outputs", "silent"])
def test_by_user_id(rs, outputs):
    """A call names a strict subset of the config's users through user_id, so that call position i is user ids[i] != i (a run's users
    ascend: a permuted list is refused, with records as without -- and moves nothing): the records carry position and id, the counters
    are the id's."""
    sched, T = 9, 3
    sc, g, twin, rng, cb, cr = _pair(rs, sched, 41, 42)
    ids = np.array([1, 2, 4, 6, 7, 10, 11], np.int32)
    now = 0.1
    for run in range(2):
        calls = [dict(cqi=synth_cqi(410 + 10 * run + k, (len(ids), R), HIST), user_id=ids, cqi_epoch=1 + run) for k in range(K)]
        nows = now + 0.001 * np.arange(1, T + 1)
        now = float(nows[-1])
        rands = _pairs(rng, K, T)
        ref = twin.run_at(calls, nows, rands)
        res, recs = g.run_counted_at(calls, nows, rands, outputs=outputs, records=True)
        if outputs:
            _same_runs(res, ref, f"7 of 12 users, run {run}")
        for k in range(K):
            _same_records(recs[k], _expected(ref[k], cb[k], cr[k], ids), f"7 of 12 users, run {run}, cell {k}")
            assert all((r["user_id"] == ids[r["pos"]]).all() for r in recs[k]) and any((r["user_id"] != r["pos"]).any() for r in recs[k])
        _same_counters(_counters(g, K), list(zip(cb, cr)), f"run {run}")
        assert _state(g, K) == _state(twin, K)
    permuted = [dict(c, user_id=ids[::-1].copy()) for c in calls]
    _refusals(rs, g, K)(-1, "ascend", lambda: g.run_counted_at(permuted, now + 0.001 * np.arange(1, T + 1), _pairs(rng, K, T), outputs=outputs, records=True))
    _same_counters(_counters(g, K), list(zip(cb, cr)), "a refused user list")
    g.close()
    twin.close()


@pytest.mark.parametrize("epoch", [4, 0])
def test_per_prb_reports_and_no_epoch(rs, epoch):
    """Per-PRB reports, under a cqi_epoch (the group copies its blocks, from TTI 1 on link adaptation reads the cell's store; the second
    run repeats the number) and under cqi_epoch 0 (every TTI reads the slot's block again): two runs without outputs."""
    sched, T = 9, 3
    sc, g, twin, rng, cb, cr = _pair(rs, sched, 31, 32)
    U = sc.n_users
    calls = [dict(cqi_prb=synth_cqi(310 + k, (U, R * G), HIST), cqi_epoch=epoch) for k in range(K)]
    now = 0.1
    for run in range(2):
        nows = now + 0.001 * np.arange(1, T + 1)
        now = float(nows[-1])
        rands = _pairs(rng, K, T)
        ref = twin.run_at(calls, nows, rands)
        res, recs = g.run_counted_at(calls, nows, rands, outputs=False, records=True)
        assert res is None
        for k in range(K):
            _same_records(recs[k], _expected(ref[k], cb[k], cr[k]), f"per-PRB reports, epoch {epoch}, run {run}, cell {k}")
        assert _state(g, K) == _state(twin, K) and g.image_stats == twin.image_stats
        _same_counters(_counters(g, K), list(zip(cb, cr)), f"per-PRB reports, run {run}")
    if epoch:
        assert g.image_stats == ((2 * T - 1) * K, K, 0)
    g.close()
    twin.close()


def test_grids_without_an_epoch(rs):
    """cqi_epoch 0 with per-RBG grids: no image, every TTI reads the slot's block; records as under a number."""
    sched, T = 10, 3
    sc, g, twin, rng, cb, cr = _pair(rs, sched, 33, 34)
    calls = _calls(K, sc.n_users, 330, epoch=0)
    nows, rands = 0.1 + 0.001 * np.arange(1, T + 1), _pairs(rng, K, T)
    ref = twin.run_at(calls, nows, rands)
    res, recs = g.run_counted_at(calls, nows, rands, records=True)
    _same_runs(res, ref, "cqi_epoch 0", upper=True)
    for k in range(K):
        _same_records(recs[k], _expected(ref[k], cb[k], cr[k]), f"cqi_epoch 0, cell {k}")
    assert _state(g, K) == _state(twin, K) and g.image_stats == twin.image_stats
    g.close()
    twin.close()


def test_a_zero_clock_step_still_has_its_records(rs):
    """now[k][1] == now[k][0]: TTI 1 updates nothing and still credits its grants -- and writes their records."""
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
    res, recs = g.run_counted_at(calls, nows, rands, outputs=False, records=True)
    one.run_counted_at(calls, nows[:1], rands[:, :1], outputs=False, records=True)
    assert res is None and _state(g, K) == _state(twin, K)
    for k in range(K):
        assert g.get_avg(k)[0].tobytes() == one.get_avg(k)[0].tobytes(), "the averages did not move in TTI 1"
        cb, cr = np.zeros(U, np.int64), np.zeros(U, np.int64)
        _same_records(recs[k], _expected(ref[k], cb, cr), f"a repeated clock value, cell {k}")
        assert len(recs[k][1]) > 0, "TTI 1 has grants"
        _same_counters([g.get_avg_counters(k)], [(cb, cr)], f"cell {k}")
    for x in (g, one, twin):
        x.close()


def test_a_subset_and_a_permutation_of_cells(rs):
    """cell_ids names cells 2 and 0, in this order: slot k's records are cell cell_ids[k]'s, cell 1 is left alone."""
    sched, T = 9, 3
    sc, g, twin, rng, cb, cr = _pair(rs, sched, 51, 52)
    before = _counters(g, K)
    cells = [2, 0]
    calls = _calls(2, sc.n_users, 510, epoch=3)
    nows, rands = 0.1 + 0.001 * np.arange(1, T + 1), _pairs(rng, 2, T)
    ref = twin.run_at(calls, nows, rands, cell_ids=cells)
    res, recs = g.run_counted_at(calls, nows, rands, cell_ids=cells, outputs=False, records=True)
    assert res is None and len(recs) == 2
    for k, cell in enumerate(cells):
        _same_records(recs[k], _expected(ref[k], cb[cell], cr[cell]), f"slot {k}, cell {cell}")
    after = _counters(g, K)
    _same_counters(after, list(zip(cb, cr)), "cells 2 and 0")
    assert after[1][0].tobytes() == before[1][0].tobytes() and after[1][1].tobytes() == before[1][1].tobytes()
    assert _state(g, K) == _state(twin, K)
    g.close()
    twin.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. log lines
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sched", [9, 10, 1])
def test_log_lines(rs, oracle, sched):
    """The reference's stderr log of the base case's three runs (T = 7), per cell: logfmt.run_record_lines on the records of the
    output-free runs against logfmt.stderr_lines fed from the twin's outputs with the same starting counters (scheduler 1: the flow:
    lines).  Scheduler 9: the counters behind the runs are the oracle's."""
    T = 7
    _, twin = _base_case(sched, T, "twin")
    start, _, got = _records_case(sched, T, False)
    slices = np.repeat(np.arange(len(UES)), UES)
    n_lines = 0
    for k in range(K):
        outs = [out for i in range(N_RUNS) for out in twin[i]["res"][k]]
        want = logfmt.stderr_lines(np.array([o.user_tbs_bits for o in outs]), np.array([o.rbg_to_user for o in outs]), slices, G, first_ts=100,
                                   cum_bytes0=start[k][0], cum_rbs0=start[k][1], nprb=np.array([o.user_nprb for o in outs]), pf_format=sched == 1)
        lines = logfmt.run_record_lines([rec for i in range(N_RUNS) for rec in got[i]["recs"][k]], slices, first_ts=100, pf_format=sched == 1)
        assert lines == want, f"sched {sched}, cell {k}"
        n_lines += len(lines)
    assert n_lines >= K * N_RUNS * T, "not vacuous: at least a line per cell-TTI"
    if sched == 9:
        ref = _oracle_counters(sched, T)
        for i in range(N_RUNS):
            _same_counters(got[i]["counters"], [(start[k][0] + ref[i][k][0], start[k][1] + ref[i][k][1]) for k in range(K)],
                           f"after run {i}, against the oracle")


# ---------------------------------------------------------------------------------------------------------------------------
# 5. rules
# ---------------------------------------------------------------------------------------------------------------------------

def test_rules(rs):
    sc = rs.SliceConfig(UES, weight=W)
    U, T = sc.n_users, 3
    g = rs.GroupScheduler(sc, R, G, K, sched=9)
    rng = np.random.default_rng(70)
    start = _start(71, K, U)
    for k in range(K):
        g.set_avg(k, rng.uniform(1e3, 5e6, U), 0.1)
    for k in (0, 1):
        g.set_avg_counters(k, *start[k])
    bound = g.grant_bound
    assert bound == min(U, R)
    calls, nows, rands = _calls(K, U, 700, epoch=1), 0.1 + 0.001 * np.arange(1, T + 1), _pairs(rng, K, T)
    two = calls[:2]
    run = rs.lib().rs_group_run_records_at
    recs, n_recs = np.zeros((2, T, bound + 3), rs.api.GRANT_RECORD), np.zeros((2, T), np.int32)
    before = (_state(g, K), _counters(g, 2))
    refused = _refusals(rs, g, K)
    for outputs in (True, False):
        # a list one short of the bound; no list; no counts
        refused(-1, "rs_group_grant_bound", lambda: g.run_counted_at(two, nows, rands[:2], outputs=outputs, records=True, rec_cap=bound - 1))
        refused(-1, "recs and n_recs", lambda: g._run(run, two, nows, rands[:2], None, outputs, rec=(bound, None, n_recs)))
        refused(-1, "recs and n_recs", lambda: g._run(run, two, nows, rands[:2], None, outputs, rec=(bound, recs, None)))
        # a cell that is not avg-counted, named by the message; the counted run's own rules come first
        refused(-4, "cell 2 is not avg-counted", lambda: g.run_counted_at(calls, nows, rands, outputs=outputs, records=True))
        refused(-1, "n_ttis", lambda: g.run_counted_at(two, 0.2 + 0.001 * np.arange(65), _pairs(rng, 2, 65), outputs=outputs, records=True))
        assert _state(g, K) == before[0]
        _same_counters(_counters(g, 2), before[1], "after the refusals")
    assert not n_recs.any() and not recs["bytes"].any(), "a refused call writes nothing"
    # a longer list is accepted; entries behind the counts keep the caller's pattern
    recs.view(np.uint8)[...] = 0xA5
    n_recs[...] = -1
    twin = rs.GroupScheduler(sc, R, G, K, sched=9)
    for k in (0, 1):
        twin.set_avg(k, g.get_avg(k)[0], 0.1)
    ref = twin.run_at(two, nows, rands[:2])
    assert g._run(run, two, nows, rands[:2], None, False, rec=(bound + 3, recs, n_recs)) is None
    assert g.launch_count == 1
    for k in (0, 1):
        cb, cr = start[k][0].copy(), start[k][1].copy()
        want = _expected(ref[k], cb, cr)
        assert [int(n) for n in n_recs[k]] == [len(w) for w in want]
        _same_records([recs[k, t, :n_recs[k, t]] for t in range(T)], want, f"a longer list, cell {k}")
        for t in range(T):
            assert (recs[k, t, n_recs[k, t]:].view(np.uint8) == 0xA5).all(), "entries behind the count were written"
    g.close()
    twin.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. with and without records, run after run
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sched", [9, 10])
def test_a_run_without_records_between_two_with(rs, sched):
    """records, no records, records on one group against three runs with records on another (both without outputs): the same state and
    counters after each, the same records in runs 0 and 2 -- the word in the slot header is per call."""
    T = 7
    a0, runs = _inputs(sched, T)
    start, bound, want = _records_case(sched, T, False)
    sc = rs.SliceConfig(UES, weight=W)
    g = rs.GroupScheduler(sc, R, G, K, sched=sched)
    for k in range(K):
        g.set_avg(k, a0[k], 0.1)
        g.set_avg_counters(k, *start[k])
    for i, run in enumerate(runs):
        if i == 1:
            assert g.run_counted_at(run["calls"], run["nows"], run["rands"], outputs=False) is None
        else:
            res, recs = g.run_counted_at(run["calls"], run["nows"], run["rands"], outputs=False, records=True)
            for k in range(K):
                _same_records(recs[k], want[i]["recs"][k], f"sched {sched} run {i} cell {k}")
        now = _record(g, K, True)
        assert now["state"] == want[i]["state"] and now["stats"] == want[i]["stats"] and now["launches"] == i + 1
        _same_counters(now["counters"], want[i]["counters"], f"sched {sched} after run {i}")
    assert g.grant_bound == bound
    g.close()
