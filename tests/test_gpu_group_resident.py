"""Resident averages of a group's cells (rs_group_set_avg / rs_group_schedule_tti_at): the device applies the reference's EWMA to every
user of the cell, schedules the TTI on the result and keeps the grants for the next update.  Against the oracle's own DoSchedule loop,
against a batch, with more users than threads, with users outside the calls, the clock rules, rs_group_set_pending, plain calls in
between, the refusals and a specialised group.  Every comparison is bitwise."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import synth_cqi
from test_gpu_group import HIST, _same

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
UES, R, G, K = [5, 4, 3], 8, 2, 3      # 3 cells; slices of 5 / 4 / 3 users; 8 RBGs of 2 PRBs
W = [0.5, 0.3, 0.2]
PER_USER = ("user_nprb", "user_final_cqi", "user_mcs", "user_tbs_bits")


def _update(avg, pending, last, now):
    """RadioBearer::UpdateAverageTransmissionRate for every user, the three operations of the header in numpy float64 (IEEE double,
    nothing fused): THIS expression is the expectation wherever a test has no oracle object beside it."""
    if now == last:
        return avg.copy()
    rate = (pending.astype(np.int32) * np.int32(8)).astype(np.float64) / (now - last)
    a = ((1 - 0.02) * avg) + (0.02 * rate)
    return np.where(a < 1, 1.0, a)


def _grants(n_users, ids, tbs_bits):
    out = np.zeros(n_users, np.int32)
    out[ids] = np.minimum(tbs_bits // 8, 100000000)
    return out


def _same_by_id(res, out, ids, what):
    """A call that names its users (`ids`) against oracle arrays that are indexed by user id: the named users' rows, nothing for the others."""
    for f in ("rbg_to_user", "target_rbs", "quota_rbgs"):
        np.testing.assert_array_equal(getattr(res, f), getattr(out, f), err_msg=f"{what}: {f}")
    others = np.setdiff1d(np.arange(len(out.user_nprb)), ids)
    for f in PER_USER:
        np.testing.assert_array_equal(getattr(res, f), getattr(out, f)[ids], err_msg=f"{what}: {f}")
        assert not getattr(out, f)[others].any(), f"{what}: the oracle served a user outside the call ({f})"


# ---------------------------------------------------------------------------------------------------------------------------
# 1. / 3. against the oracle's own DoSchedule loop
# ---------------------------------------------------------------------------------------------------------------------------

def _against_the_oracle(rs, oracle, sched, ues, w, n_rbgs, n_cells, n_ttis, renew, seed, check_at):
    sc = rs.SliceConfig(ues, weight=w)
    U, u2s = sc.n_users, np.asarray(sc.user_to_slice)
    g = rs.GroupScheduler(sc, n_rbgs, G, n_cells, sched=sched)
    cells = [oracle.Cell(ues, n_rbgs, G, sched, weights=w) for _ in range(n_cells)]
    ticks = oracle.clock_ticks(100, n_ttis)
    rands = [oracle.Rng(seed + 17 * k) for k in range(n_cells)]   # (the glibc rand() restatement)
    rng = np.random.default_rng(seed)
    for k in range(n_cells):  # per cell its own seed, grids and starting averages; bearers created at 0.1 s as in the reference's runs
        a0 = rng.uniform(1e3, 5e6, U)
        cells[k].set_avg_rate(a0)
        cells[k].set_last_update(0.1)
        g.set_avg(k, a0, 0.1)
    cqi = [None] * n_cells
    for it in range(n_ttis):
        calls, outs, ids_of = [], [], []
        for k in range(n_cells):
            if it % renew == 0:
                cqi[k] = synth_cqi(seed + 1000 * k + it, (U, n_rbgs), HIST)
                cells[k].set_cqi(cqi[k])
            r0, r1 = rands[k].rand(), rands[k].rand()
            out = cells[k].new_out()
            assert cells[k].step(float(ticks[it]), r0, r1, out) == 0
            outs.append(out)
            kw = dict(cqi=cqi[k], rand0=r0, rand1=r1, cqi_epoch=1 + it // renew)
            ids = None
            if sched == 7:  # the call's users are those of the slice the oracle's NVS step served
                ids = np.flatnonzero(u2s == out.served_slice).astype(np.int32)
                kw.update(cqi=cqi[k][ids], user_id=ids)
            ids_of.append(ids)
            calls.append(kw)
        res = g.schedule_tti_at(calls, ticks[it])
        for k in range(n_cells):
            what = f"sched {sched} TTI {it} cell {k}"
            if ids_of[k] is None:
                _same(res[k], outs[k], what)
            else:
                _same_by_id(res[k], outs[k], ids_of[k], what)
        if it + 1 in check_at:
            for k in range(n_cells):
                a, _, last = g.get_avg(k)
                assert a.tobytes() == cells[k].state()["avg_rate"].tobytes(), f"sched {sched} after TTI {it + 1}, cell {k}: averages"
                assert last == ticks[it]
    assert g.launch_count == n_ttis
    if sched != 7:  # one store per renewal, every other call from the cell's image: the reuse counts of a resident stream
        n_store = (n_ttis + renew - 1) // renew
        assert g.image_stats == ((n_ttis - n_store) * n_cells, n_store * n_cells, 0)
    g.close()


@pytest.mark.parametrize("sched", [1, 7, 8, 9])
def test_against_the_oracle(rs, oracle, sched):
    """60 TTIs, new CQI grids (and a new cqi_epoch) every 10, the clock of the oracle's run loops, rand0 / rand1 from the glibc rand()
    restatement: every rs_tti_out field of every TTI, and the averages after TTIs 1, 2, 30 and 60 (54 of 60 calls per cell served
    from the cell's CQI image)."""
    _against_the_oracle(rs, oracle, sched, UES, W, R, K, 60, 10, 4100 + sched, check_at=(1, 2, 30, 60))


def test_more_users_than_threads(rs, oracle):
    """One slice pair of 700 users, 4 RBGs, 20 TTIs: the strided update and the gather cover users beyond the workgroup's size."""
    _against_the_oracle(rs, oracle, 9, [350, 350], [0.5, 0.5], 4, 2, 20, 10, 5200, check_at=(1, 20))


# ---------------------------------------------------------------------------------------------------------------------------
# 2. against a batch: two product paths that share no host code
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sched", [9, 7])
def test_against_a_batch(rs, oracle, sched):
    n_ttis, renew = 60, 10
    sc = rs.SliceConfig(UES, weight=W)
    U, u2s = sc.n_users, np.asarray(sc.user_to_slice)
    rng = np.random.default_rng(6100 + sched)
    grids = np.stack([np.stack([synth_cqi(6100 + 100 * k + e, (U, R), HIST) for e in range(n_ttis // renew)]) for k in range(K)])
    seeds = np.arange(K, dtype=np.uint32) + 77
    a0 = rng.uniform(1e3, 5e6, (K, U))
    b = rs.BatchScheduler(sc, R, G, K, sched=sched, cqi_refresh=renew)   # first TTI: tick 100, bearers' m_lastUpdate 0.1
    b.upload_cqi_epochs(grids)
    b.seed(seeds)
    b.write_state(avg_rate=a0)
    log = b.run_logged(n_ttis)
    final = b.state()["avg_rate"]
    b.close()
    g = rs.GroupScheduler(sc, R, G, K, sched=sched)
    ticks = oracle.clock_ticks(100, n_ttis)
    rands = [oracle.Rng(int(s)) for s in seeds]
    for k in range(K):
        g.set_avg(k, a0[k], 0.1)
    for it in range(n_ttis):
        calls, ids_of = [], []
        for k in range(K):
            kw = dict(cqi=grids[k, it // renew], cqi_epoch=1 + it // renew)
            ids = np.arange(U, dtype=np.int32)
            if sched == 9:
                kw.update(rand0=rands[k].rand(), rand1=rands[k].rand())
            else:  # the slice the batch's NVS step served is the one its allocation went to
                served = log["rbg_to_user"][k, it]
                assert (served >= 0).any()
                ids = np.flatnonzero(u2s == u2s[served[served >= 0][0]]).astype(np.int32)
                kw.update(cqi=kw["cqi"][ids], user_id=ids)
            ids_of.append(ids)
            calls.append(kw)
        res = g.schedule_tti_at(calls, ticks[it])
        for k in range(K):
            what, ids = f"sched {sched} TTI {it} cell {k}", ids_of[k]
            np.testing.assert_array_equal(res[k].rbg_to_user, log["rbg_to_user"][k, it], err_msg=what)
            for mine, theirs in (("user_tbs_bits", "tbs_bits"), ("user_nprb", "nprb"), ("user_final_cqi", "final_cqi"), ("user_mcs", "mcs")):
                full = np.zeros(U, np.int64)
                full[ids] = getattr(res[k], mine)
                np.testing.assert_array_equal(full, log[theirs][k, it], err_msg=f"{what}: {mine}")
    for k in range(K):
        assert g.get_avg(k)[0].tobytes() == final[k].tobytes(), f"sched {sched} cell {k}: the averages at the end"
    g.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. users without data
# ---------------------------------------------------------------------------------------------------------------------------

def _named_users(rs, ues, w, n_rbgs, n_named, n_ttis, seed):
    """Calls that name `n_named` of the cell's users through user_id, another set on every TTI, against a plain group fed the averages
    that get_avg returned just before, put through _update."""
    sc = rs.SliceConfig(ues, weight=w)
    U, n_cells = sc.n_users, 2
    g = rs.GroupScheduler(sc, n_rbgs, G, n_cells, sched=9)
    plain = rs.GroupScheduler(sc, n_rbgs, G, n_cells, sched=9)
    rng = np.random.default_rng(seed)
    for k in range(n_cells):
        g.set_avg(k, rng.uniform(1.0, 3e4, U), 0.5)   # (small averages: the decay of an idle user reaches the clamp at 1)
    now = 0.5
    for it in range(n_ttis):
        now += 0.001 * (1 + it % 3)
        calls, want, ids_of = [], [], []
        for k in range(n_cells):
            ids = np.sort(rng.choice(U, n_named, replace=False)).astype(np.int32)
            a, pend, last = g.get_avg(k)
            want.append(_update(a, pend, last, now))
            ids_of.append(ids)
            calls.append(dict(cqi=synth_cqi(seed + 10 * it + k, (n_named, n_rbgs), HIST), user_id=ids, rand0=int(rng.integers(0, 2**31 - 1)),
                              rand1=int(rng.integers(0, 2**31 - 1))))
        res = g.schedule_tti_at(calls, now)
        ref = plain.schedule_tti([dict(c, avg_rate=want[k][ids_of[k]]) for k, c in enumerate(calls)])
        for k in range(n_cells):
            _same(res[k], ref[k], f"TTI {it} cell {k}")
            a, pend, last = g.get_avg(k)
            assert a.tobytes() == want[k].tobytes(), f"TTI {it} cell {k}: averages, named or not"
            np.testing.assert_array_equal(pend, _grants(U, ids_of[k], res[k].user_tbs_bits), err_msg=f"TTI {it} cell {k}: pending bytes")
            assert last == now
            assert plain.slice_offset(k).tobytes() == g.slice_offset(k).tobytes()
    g.close()
    plain.close()


def test_users_without_data(rs):
    """12 users, calls that name 7 of them, another 7 on every TTI.  Outputs equal a plain rs_group_schedule_tti fed the averages that
    get_avg returned just before, put through _update; the averages of the users outside the calls follow _update with zero bytes --
    the numpy float64 expression is the expectation here."""
    _named_users(rs, UES, W, R, 7, 20, 800)


def test_more_named_users_than_threads(rs):
    """700 users, calls that name 600 of them: a user_id list longer than the workgroup, so the gather, the ids kept for the grants and
    the grants' scatter all run at positions beyond the workgroup's size (the kernels have at most 512 threads)."""
    _named_users(rs, [350, 350], [0.5, 0.5], 4, 600, 6, 900)


def test_copy_path_in_a_fresh_process():
    """The tests above once more without zero-copy slots (RS_DROPIN_COPY=1 is read when a group is created): a child process."""
    me = "tests/test_gpu_group_resident.py::"
    ids = [me + t for t in ("test_against_the_oracle", "test_more_users_than_threads", "test_against_a_batch", "test_users_without_data",
                            "test_more_named_users_than_threads")]
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider"] + ids, cwd=ROOT,
                       env=dict(os.environ, RS_DROPIN_COPY="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]


# ---------------------------------------------------------------------------------------------------------------------------
# 5. - 8. clock rules, set_pending, coexistence, refusals
# ---------------------------------------------------------------------------------------------------------------------------

def _plain_calls(rng, n_cells, U, seed):
    return [dict(cqi=synth_cqi(seed + k, (U, R), HIST), rand0=int(rng.integers(0, 2**31 - 1)), rand1=int(rng.integers(0, 2**31 - 1)))
            for k in range(n_cells)]


def _state(g, n_cells):
    return [tuple(x.tobytes() if isinstance(x, np.ndarray) else x for x in g.get_avg(k)) for k in range(n_cells)]


def test_clock_rules(rs):
    sc = rs.SliceConfig(UES, weight=W)
    U = sc.n_users
    g = rs.GroupScheduler(sc, R, G, 1, sched=9)
    rng = np.random.default_rng(5)
    a0 = rng.uniform(1e3, 5e6, U)
    g.set_avg(0, a0, 0.25)
    r1 = g.schedule_tti_at(_plain_calls(rng, 1, U, 50), 0.25)[0]   # now == last_update, twice in a row: the reference's early return
    r2 = g.schedule_tti_at(_plain_calls(rng, 1, U, 60), 0.25)[0]
    a, pend, last = g.get_avg(0)
    assert a.tobytes() == a0.tobytes() and last == 0.25
    both = _grants(U, np.arange(U), r1.user_tbs_bits) + _grants(U, np.arange(U), r2.user_tbs_bits)
    assert both.any()
    np.testing.assert_array_equal(pend, both)
    launches, before = g.launch_count, _state(g, 1)
    for bad in (0.2499, float("nan"), float("inf"), 0.25 + 2.0**-30):   # before the last update; not finite; bytes pending and too close
        with pytest.raises(rs.RadioSaberError) as e:
            g.schedule_tti_at(_plain_calls(rng, 1, U, 70), bad)
        assert e.value.code == -1, str(e.value)   # RS_ERR_INVALID
        assert g.launch_count == launches and _state(g, 1) == before
    g.schedule_tti_at(_plain_calls(rng, 1, U, 80), 0.251)
    a, _, last = g.get_avg(0)
    assert a.tobytes() == _update(a0, both, 0.25, 0.251).tobytes() and last == 0.251
    g.close()


def test_set_pending(rs):
    sc = rs.SliceConfig(UES, weight=W)
    U = sc.n_users
    g = rs.GroupScheduler(sc, R, G, 1, sched=9)
    rng = np.random.default_rng(6)
    g.set_avg(0, rng.uniform(1e3, 5e6, U), 1.0)
    g.schedule_tti_at(_plain_calls(rng, 1, U, 90), 1.001)
    a, pend, last = g.get_avg(0)
    u = int(np.flatnonzero(pend)[0])
    credited = pend.copy()
    credited[u] = pend[u] // 3   # a finite queue held less than the transport block
    g.set_pending(0, credited)
    assert g.get_avg(0)[1].tolist() == credited.tolist()
    g.schedule_tti_at(_plain_calls(rng, 1, U, 95), 1.002)
    want = _update(a, credited, last, 1.002)
    assert want[u] != _update(a, pend, last, 1.002)[u]
    assert g.get_avg(0)[0].tobytes() == want.tobytes()
    with pytest.raises(rs.RadioSaberError):
        g.set_pending(0, -credited - 1)
    g.close()


def test_coexistence_with_plain_calls_subsets_and_permutations(rs):
    sc = rs.SliceConfig(UES, weight=W)
    U = sc.n_users
    g = rs.GroupScheduler(sc, R, G, K, sched=9)
    rng = np.random.default_rng(7)
    for k in range(K):
        g.set_avg(k, rng.uniform(1e3, 5e6, U), 2.0)
    g.schedule_tti_at(_plain_calls(rng, K, U, 100), 2.001)
    # a plain call between two resident ones: the caller's averages, the resident state neither read nor written
    before = _state(g, K)
    fresh = rs.GroupScheduler(sc, R, G, K, sched=9)
    for k in range(K):
        fresh.set_slice_offset(k, g.slice_offset(k))
    calls = [dict(c, avg_rate=rng.uniform(1e3, 5e6, U)) for c in _plain_calls(rng, K, U, 110)]
    mine, theirs = g.schedule_tti(calls), fresh.schedule_tti(calls)
    for k in range(K):
        _same(mine[k], theirs[k], f"plain call, cell {k}")
    assert _state(g, K) == before
    assert g.kernel_name.startswith("rs_group_kernel<9,")

    def resident(cells, now, seed):
        """A resident call naming `cells` in this order, against `fresh` fed the expected averages; the other cells' state must not move."""
        untouched = {k: _state(g, K)[k] for k in range(K) if k not in cells}
        nows = np.broadcast_to(np.asarray(now, np.float64), (len(cells),))
        want = {k: _update(*g.get_avg(k), float(nows[j])) for j, k in enumerate(cells)}
        calls = _plain_calls(rng, len(cells), U, seed)
        for k in cells:
            fresh.set_slice_offset(k, g.slice_offset(k))
        res = g.schedule_tti_at(calls, now, cell_ids=cells)
        ref = fresh.schedule_tti([dict(c, avg_rate=want[k]) for c, k in zip(calls, cells)], cell_ids=cells)
        for j, k in enumerate(cells):
            _same(res[j], ref[j], f"cells {cells}: cell {k} in slot {j}")
            a, _, last = g.get_avg(k)
            assert a.tobytes() == want[k].tobytes() and last == nows[j]
        for k, st in untouched.items():
            assert _state(g, K)[k] == st, f"cells {cells}: cell {k} was not named"   # averages, pending bytes AND last_update

    resident([0, 1, 2], 2.002, 120)
    assert g.kernel_name.startswith("rs_group_resident_kernel<9,")
    resident([2, 0, 1], 2.003, 130)   # a permutation
    resident([1, 2], 2.004, 140)      # 2 of 3 ...
    resident([0], 2.005, 150)         # ... and the third, two ticks behind its last update
    resident([1, 0, 2], np.array([2.006, 2.007, 2.0055]), 160)   # a clock per cell
    g.close()
    fresh.close()


def test_refusals(rs):
    sc = rs.SliceConfig(UES, weight=W)
    U = sc.n_users
    g = rs.GroupScheduler(sc, R, G, 2, sched=9)
    rng = np.random.default_rng(9)
    good = rng.uniform(1e3, 5e6, U)
    g.set_avg(0, good, 0.1)

    def refused(code, frag, fn):
        launches = g.launch_count
        with pytest.raises(rs.RadioSaberError) as e:
            fn()
        assert e.value.code == code and frag in str(e.value), str(e.value)
        assert g.launch_count == launches

    refused(-4, "cell 1", lambda: g.schedule_tti_at(_plain_calls(rng, 2, U, 200), 0.101))   # RS_ERR_STATE: cell 1 is not resident
    refused(-4, "not resident", lambda: g.get_avg(1))
    refused(-1, "avg_rate", lambda: g.schedule_tti_at([dict(c, avg_rate=good) for c in _plain_calls(rng, 1, U, 210)], 0.101))
    refused(-1, "avg[3]", lambda: g.set_avg(1, np.where(np.arange(U) == 3, 0.5, good), 0.1))
    refused(-1, "avg[0]", lambda: g.set_avg(1, np.where(np.arange(U) == 0, np.nan, good), 0.1))
    refused(-1, "avg_rate", lambda: g.schedule_tti([dict(c, avg_rate=None) for c in _plain_calls(rng, 1, U, 220)]))   # the plain call still needs its averages
    a, pend, last = g.get_avg(0)
    assert a.tobytes() == good.tobytes() and not pend.any() and last == 0.1
    g.close()
    sq = rs.SliceConfig(UES, weight=W, algo_epsilon=[1, 2, 1], algo_psi=[1, 1, 1])   # an exponent of 2
    g = rs.GroupScheduler(sq, R, G, 1, sched=9)
    g.set_avg(0, good, 0.1)
    refused(-1, "exponents", lambda: g.schedule_tti_at(_plain_calls(rng, 1, U, 230), 0.101))
    g.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 9. after rs_group_specialize
# ---------------------------------------------------------------------------------------------------------------------------

def test_after_specialize(rs):
    """Resident calls of a specialised group run the built-in resident kernel and return what they returned before; plain calls still
    run the group's own builds."""
    sc = rs.SliceConfig(UES, weight=W)
    U = sc.n_users
    groups = [rs.GroupScheduler(sc, R, G, K, sched=9), rs.GroupScheduler(sc, R, G, K, sched=9, jit=True)]
    assert groups[1].jit_status()[0] == 1
    rng = np.random.default_rng(10)
    a0 = [rng.uniform(1e3, 5e6, U) for _ in range(K)]
    for g in groups:
        for k in range(K):
            g.set_avg(k, a0[k], 0.1)
    for it in range(6):
        calls = _plain_calls(rng, K, U, 300 + 10 * it)
        if it % 3 == 2:   # a plain call in between
            calls = [dict(c, avg_rate=a0[k]) for k, c in enumerate(calls)]
            res = [g.schedule_tti(calls) for g in groups]
            assert groups[1].kernel_name == "rs_group_kernel_jit"
        else:
            res = [g.schedule_tti_at(calls, 0.101 + 0.001 * it) for g in groups]
            assert groups[1].kernel_name == groups[0].kernel_name and groups[1].kernel_name.startswith("rs_group_resident_kernel<9,")
        for k in range(K):
            _same(res[1][k], res[0][k], f"call {it} cell {k}")
    for k in range(K):
        assert _state(groups[0], K)[k] == _state(groups[1], K)[k]
    assert groups[1].jit_status()[0] == 1
    for g in groups:
        g.close()
