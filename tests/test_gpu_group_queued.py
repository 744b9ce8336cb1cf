"""Resident bearers of a group's cells (rs_group_set_bearers / rs_group_schedule_tti_queued): the device keeps both bearers of every user
-- average, bytes credited since the last update, existence --, applies the reference's EWMA to every existing bearer, schedules
the TTI on the sums over the bearers with data and credits DoStopSchedule's min(available, dataToTransmit) per bearer.

Checked against the oracle's DoSchedule() with queues (rso_cell_step_queues: UNPINNED, tests/PINS.md -- these tests prove device ==
oracle), against a numpy restatement of the three host-visible steps on a plain-call twin, and against the resident-averages call
in the case where both forms must agree.  Every comparison is bitwise.  The scenario and the proof that it binds (finite credits,
split grants, idle cells) are tests/test_group_queued_abi.py's."""
import numpy as np
import pytest

from conftest import synth_cqi
from test_group_queued_abi import CELLS, FIELDS, G_SMALL, HIST, INFINITE, PER_USER, R_SMALL, UES, credit, oracle_run

BITS = lambda a: np.ascontiguousarray(a).tobytes()  # noqa: E731


def make_group(rs, sched, ues=UES, R=R_SMALL, G=G_SMALL, K=CELLS, **cfg):
    return rs.GroupScheduler(rs.SliceConfig(ues, **cfg), R, G, K, sched=sched)


def device_calls(sched, row):
    """One TTI's records of oracle_run as the calls of schedule_tti_queued: the active users, or an update-only slot."""
    calls = []
    for st in row:
        if len(st["ids"]) == 0:
            calls.append(dict(n_users=0))
            continue
        kw = dict(cqi=st["cqi"], user_id=st["ids"], data_to_transmit=st["data"], cqi_epoch=st["epoch"])
        if st["rand"] is not None:
            kw.update(rand0=st["rand"][0], rand1=st["rand"][1])
        if sched == 7:
            kw.update(required_rbs=st["required_rbs"])
        calls.append(kw)
    return calls


def same_as_oracle(res, st, S, R, what):
    out, ids = st["out"], st["ids"]
    for f in FIELDS:
        want = getattr(out, f)
        np.testing.assert_array_equal(getattr(res, f), want[ids] if f in PER_USER else want, err_msg=f"{what}: {f}")


def follow_the_oracle(g, run, sched, what, collect=None):
    """The device along oracle_run's record: every rs_tti_out field every TTI, the bearers' averages at the recorded TTIs."""
    K, U = len(run["kinds"]), len(run["kinds"][0])
    S = g.slices.n_slices
    for k in range(K):
        g.set_bearers(k, run["kinds"][k] != 0, np.full((U, 2), 100000.0), 0.1)
    for t, row in enumerate(run["steps"]):
        res = g.schedule_tti_queued(device_calls(sched, row), run["ticks"][t])
        for k in range(K):
            same_as_oracle(res[k], row[k], S, g.R, f"{what} TTI {t} cell {k}")
            if collect is not None:
                collect.append(b"".join(BITS(getattr(res[k], f)) for f in FIELDS))
        if t + 1 in run["state"]:
            for k in range(K):
                avg, _, last = g.get_bearers(k)
                has = run["kinds"][k] != 0
                assert BITS(avg[has]) == BITS(run["state"][t + 1][k][has]), f"{what}: averages of cell {k} after TTI {t + 1}"
                assert not avg[~has].any(), f"{what}: a bearer that does not exist reports an average"
                assert last == run["ticks"][t]
                if collect is not None:
                    collect.append(BITS(avg))


# ---- 3. against the oracle's DoSchedule() with queues ----

@pytest.mark.gpu
@pytest.mark.parametrize("sched", [8, 9, 7, 103])
def test_queued_calls_against_the_oracle(rs, oracle, sched):
    run = oracle_run(oracle, sched)
    g = make_group(rs, sched)
    follow_the_oracle(g, run, sched, f"sched {sched}")
    assert g.kernel_name.startswith(f"rs_group_queued_kernel<{sched},")
    g.close()


# ---- 4. more bearers than threads ----

@pytest.mark.gpu
def test_more_bearers_than_threads(rs, oracle):
    """2 x 350 users: the strided update covers 1 400 bearers, the gather up to 700 call positions."""
    kw = dict(ues=[350, 350], R=4, G=2, K=2)
    run = oracle_run(oracle, 9, n_tti=12, grid_every=5, seed=3, busy=0.5, state_at=(1, 2, 12), **kw)
    assert max(len(st["ids"]) for row in run["steps"] for st in row) > 512
    g = make_group(rs, 9, **kw)
    follow_the_oracle(g, run, 9, "700 users")
    g.close()


# ---- 5. a customised slice against a plain-call twin fed by a numpy restatement ----

def numpy_update(avg, pend, has, now, last):
    """step 1 on [U][2] arrays (numpy evaluates operation by operation: nothing is fused)"""
    if now == last:
        return
    rate = (pend * np.int32(8)).astype(np.int32).astype(np.float64) / (now - last)
    a = ((1 - 0.02) * avg) + (0.02 * rate)
    a = np.where(a < 1, 1.0, a)
    avg[has] = a[has]
    pend[has] = 0


def numpy_sums(avg, ids, data):
    both = (data[:, 0] > 0) & (data[:, 1] > 0)
    one = np.where(data[:, 0] > 0, avg[ids, 0], avg[ids, 1])
    return np.where(both, ((1 + avg[ids, 0]) + avg[ids, 1]) - 1, one)


@pytest.mark.gpu
def test_customised_slices_against_a_plain_twin(rs):
    sched, K, U = 9, CELLS, sum(UES)
    cfg = dict(algo_alpha=[1, 1, 1], algo_beta=[1, 1, 1])
    g, twin = make_group(rs, sched, **cfg), make_group(rs, sched, **cfg)
    rng = np.random.default_rng(55)
    has = [rng.random((U, 2)) < 0.75 for _ in range(K)]
    for h in has:
        h[~h.any(axis=1), 0] = True
    avg = [np.where(h, rng.uniform(1e3, 5e6, (U, 2)), 0.0) for h in has]
    pend = [np.zeros((U, 2), np.int32) for _ in range(K)]
    last = [0.1] * K
    for k in range(K):
        g.set_bearers(k, has[k], avg[k], last[k])
    splits = 0
    for t in range(30):
        now = 0.1 + 0.001 * (t + 1) if t % 7 else last[0]  # every seventh call repeats the clock: no update, the credits pile up
        calls, plain = [], []
        for k in range(K):
            numpy_update(avg[k], pend[k], has[k], now, last[k])
            last[k] = now
            data = np.where(has[k], rng.choice(np.array([0, 0, 37, 300, 2000, INFINITE], np.int32), (U, 2)), 0).astype(np.int32)
            ids = np.nonzero(data.any(axis=1))[0].astype(np.int32)
            if len(ids) == 0:
                ids = np.array([0], np.int32)
                data[0, np.argmax(has[k][0])] = 500
            n = len(ids)
            common = dict(cqi=synth_cqi(5000 + 10 * t + k, (n, R_SMALL), HIST), user_id=ids, rand0=int(rng.integers(0, 2**31 - 1)),
                          rand1=int(rng.integers(0, 2**31 - 1)), hol_delay=rng.uniform(1e-5, 0.4, n),
                          prio_has_data=(rng.random(n) < 0.8).astype(np.uint8))
            calls.append(dict(common, data_to_transmit=data[ids]))
            plain.append(dict(common, avg_rate=numpy_sums(avg[k], ids, data[ids])))
        res, want = g.schedule_tti_queued(calls, now), twin.schedule_tti(plain)
        for k in range(K):
            for f in FIELDS:
                np.testing.assert_array_equal(getattr(res[k], f), getattr(want[k], f), err_msg=f"TTI {t} cell {k}: {f}")
            ids, data = calls[k]["user_id"], calls[k]["data_to_transmit"]
            for i, u in enumerate(ids):
                sent = credit(want[k].user_tbs_bits[i], data[i])
                pend[k][u] += np.array(sent, np.int32)
                splits += sent[0] > 0 and sent[1] > 0
            a, p, l = g.get_bearers(k)
            assert BITS(a) == BITS(avg[k]), f"TTI {t} cell {k}: averages"
            assert BITS(p) == BITS(pend[k]), f"TTI {t} cell {k}: pending bytes"
            assert l == now
            assert BITS(g.slice_offset(k)) == BITS(twin.slice_offset(k))
    assert splits > 0
    g.close()
    twin.close()


# ---- 6. the degenerate case equals the existing resident call ----

@pytest.mark.gpu
@pytest.mark.parametrize("sched", [9, 7])
def test_one_infinite_bearer_per_user_equals_the_resident_call(rs, sched):
    K, U = CELLS, sum(UES)
    first = np.concatenate([[0], np.cumsum(UES)])
    g, twin = make_group(rs, sched), make_group(rs, sched)
    rng = np.random.default_rng(66 + sched)
    has = np.zeros((U, 2), bool)
    has[:, 0] = True
    for k in range(K):
        a0 = rng.uniform(1e3, 5e6, U)
        g.set_bearers(k, has, np.stack([a0, np.zeros(U)], axis=1), 0.1)
        twin.set_avg(k, a0, 0.1)
    for t in range(40):
        now = 0.1 + 0.001 * (t + 1)
        calls = []
        for k in range(K):
            ids = np.arange(first[(t + k) % 3], first[(t + k) % 3 + 1], dtype=np.int32) if sched == 7 else np.arange(U, dtype=np.int32)
            calls.append(dict(cqi=synth_cqi(6000 + 10 * t + k, (len(ids), R_SMALL), HIST), user_id=ids,
                              rand0=int(rng.integers(0, 2**31 - 1)), rand1=int(rng.integers(0, 2**31 - 1)), cqi_epoch=1 + t // 10))
        res = g.schedule_tti_queued([dict(c, data_to_transmit=np.tile(np.array([INFINITE, 0], np.int32), (len(c["user_id"]), 1))) for c in calls], now)
        want = twin.schedule_tti_at(calls, now)
        for k in range(K):
            for f in FIELDS:
                np.testing.assert_array_equal(getattr(res[k], f), getattr(want[k], f), err_msg=f"sched {sched} TTI {t} cell {k}: {f}")
            (a, p, l), (ta, tp, tl) = g.get_bearers(k), twin.get_avg(k)
            assert BITS(a[:, 0]) == BITS(ta) and BITS(p[:, 0]) == BITS(tp) and l == tl, f"sched {sched} TTI {t} cell {k}: resident state"
            assert not a[:, 1].any() and not p[:, 1].any()
    g.close()
    twin.close()


# ---- 7. update-only slots ----

def simple_call(rng, seed, ids=None, n=None, data=None):
    n = len(ids) if ids is not None else n
    kw = dict(cqi=synth_cqi(seed, (n, R_SMALL), HIST), rand0=int(rng.integers(0, 2**31 - 1)), rand1=int(rng.integers(0, 2**31 - 1)),
              data_to_transmit=np.tile(np.array([700, 0], np.int32), (n, 1)) if data is None else data)
    if ids is not None:
        kw["user_id"] = np.asarray(ids, np.int32)
    return kw


def whole_state(g, cells=range(CELLS), counters=True):
    """everything a rejected call must leave alone, as bytes"""
    parts = []
    for k in cells:
        parts.append(BITS(g.slice_offset(k)))
        try:
            a, p, l = g.get_bearers(k)
        except Exception:
            try:
                a, p, l = g.get_avg(k)
            except Exception:
                a, p, l = np.zeros(0), np.zeros(0), -1.0
        parts += [BITS(a), BITS(p), np.float64(l).tobytes()]
    return b"".join(parts) + (repr((g.launch_count, g.image_stats)).encode() if counters else b"")


@pytest.mark.gpu
def test_update_only_slots(rs):
    U = sum(UES)
    g = make_group(rs, 9)
    rng = np.random.default_rng(7)
    has = np.ones((U, 2), bool)
    has[3] = (True, False)
    for k in range(CELLS):
        g.set_bearers(k, has, np.full((U, 2), 2e5), 0.1)
    g.schedule_tti_queued([simple_call(rng, 70 + k, n=U) for k in range(CELLS)], 0.101)
    before = [g.get_bearers(k) for k in range(CELLS)]
    assert all(b[1].any() for b in before)
    offs, stats, launches = [g.slice_offset(k).copy() for k in range(CELLS)], g.image_stats, g.launch_count
    # a mixed call: cell 1 has nobody to schedule
    res = g.schedule_tti_queued([simple_call(rng, 80, n=U), dict(n_users=0), simple_call(rng, 82, n=U)], 0.102)
    assert (res[1].rbg_to_user == -1).all() and not res[1].target_rbs.any() and not res[1].quota_rbgs.any() and len(res[1].user_tbs_bits) == 0
    assert (res[0].rbg_to_user >= 0).any()
    assert BITS(g.slice_offset(1)) == BITS(offs[1])
    assert g.image_stats == (stats[0], stats[1], stats[2] + 2) and g.launch_count == launches + 1
    a, p, l = g.get_bearers(1)
    want_a, want_p = before[1][0].copy(), before[1][1].copy()
    numpy_update(want_a, want_p, has, 0.102, 0.101)
    assert BITS(a) == BITS(want_a) and BITS(a) != BITS(before[1][0]) and not p.any() and l == 0.102
    # all slots empty, named out of order: still one launch, every cell's update is done
    launches = g.launch_count
    g.schedule_tti_queued([dict(n_users=0)] * CELLS, [0.103, 0.104, 0.105], cell_ids=[2, 0, 1])
    assert g.launch_count == launches + 1
    assert [g.get_bearers(k)[2] for k in range(CELLS)] == [0.104, 0.105, 0.103]
    assert not any(g.get_bearers(k)[1].any() for k in range(CELLS))
    # the same clock again: nothing moves
    state = whole_state(g, counters=False)
    g.schedule_tti_queued([dict(n_users=0)], [0.104], cell_ids=[0])
    assert whole_state(g, counters=False) == state
    # the other calls take no empty slot
    with pytest.raises(rs.RadioSaberError):
        g.schedule_tti([dict(cqi=np.zeros((0, R_SMALL), np.uint8), avg_rate=np.zeros(0))])
    g.close()


# ---- 8. refusals ----

@pytest.mark.gpu
def test_set_bearers_refusals(rs):
    U = sum(UES)
    has, avg = np.ones((U, 2), bool), np.full((U, 2), 1e5)
    for sched in (1, 10):
        g = make_group(rs, sched)
        with pytest.raises(rs.RadioSaberError, match="not served"):
            g.set_bearers(0, has, avg, 0.1)
        g.close()
    cfg = rs.SliceConfig([sum(UES)])
    with pytest.raises(rs.RadioSaberError):  # (a group does not serve scheduler 11 at all)
        rs.GroupScheduler(cfg, R_SMALL, G_SMALL, 1, sched=11)
    g = make_group(rs, 9, algo_epsilon=[2, 1, 1])
    with pytest.raises(rs.RadioSaberError, match="exponents"):
        g.set_bearers(0, has, avg, 0.1)
    g.close()
    g = make_group(rs, 9)
    for bad in (0.5, 2.0**51 * 1.5, np.nan, np.inf):
        a = avg.copy()
        a[4, 1] = bad
        with pytest.raises(rs.RadioSaberError, match="outside 1..2\\^51"):
            g.set_bearers(0, has, a, 0.1)
        h = has.copy()
        h[4, 1] = False
        g.set_bearers(0, h, a, 0.1)  # the average of a bearer that does not exist is not read
        assert g.get_bearers(0)[0][4, 1] == 0
    for bad in (np.nan, np.inf):
        with pytest.raises(rs.RadioSaberError, match="finite"):
            g.set_bearers(1, has, avg, bad)
    a = avg.copy()
    a[0, 0], a[0, 1] = 2.0**51, 1.0
    g.set_bearers(1, has, a, 0.1)  # the ends of the range
    g.set_bearers(2, np.zeros((U, 2), bool), avg, 0.1)  # no bearer at all
    assert not g.get_bearers(2)[0].any()
    with pytest.raises(rs.RadioSaberError):
        g.set_bearers(3, has, avg, 0.1)
    g.close()


@pytest.mark.gpu
def test_queued_call_refusals_move_nothing(rs):
    U = sum(UES)
    g = make_group(rs, 9)
    rng = np.random.default_rng(8)
    has = np.ones((U, 2), bool)
    has[2, 1] = False
    g.set_bearers(0, has, np.full((U, 2), 3e5), 0.1)
    g.set_bearers(1, has, np.full((U, 2), 4e5), 0.1)
    g.set_avg(2, np.full(U, 5e5), 0.1)
    g.schedule_tti_queued([simple_call(rng, 90 + k, n=U) for k in range(2)], 0.101, cell_ids=[0, 1])
    g.schedule_tti_at([dict(cqi=synth_cqi(95, (U, R_SMALL), HIST))], 0.101, cell_ids=[2])
    state = whole_state(g)
    ok = lambda **kw: dict(simple_call(rng, 99, n=U), **kw)  # noqa: E731

    def refused(code, match, calls, now, ids, fn=None):
        with pytest.raises(rs.RadioSaberError, match=match) as e:
            (fn or g.schedule_tti_queued)(calls, now, cell_ids=ids)
        assert e.value.code == code, e.value
        assert whole_state(g) == state, f"a rejected call moved something ({match})"

    d = np.tile(np.array([700, 0], np.int32), (U, 1))
    refused(-1, "avg_rate must be NULL", [ok(avg_rate=np.ones(U))], 0.102, [0])
    refused(-4, "not bearer-resident", [ok()], 0.102, [2])
    refused(-4, "bearer-resident", [dict(cqi=synth_cqi(96, (U, R_SMALL), HIST))], 0.102, [0], fn=g.schedule_tti_at)
    refused(-1, "before the cell's last update", [ok()], 0.1005, [0])
    refused(-1, "not finite", [ok()], np.nan, [0])
    refused(-1, "neither 0 nor at least", [ok()], 0.101 + 2.0**-24, [0])
    neg = d.copy(); neg[5, 0] = -1
    refused(-1, "negative", [ok(data_to_transmit=neg)], 0.102, [0])
    none = d.copy(); none[7] = 0
    refused(-1, "no data in either bearer", [ok(data_to_transmit=none)], 0.102, [0])
    ghost = d.copy(); ghost[2, 1] = 10
    refused(-1, "has no bearer of priority 1", [ok(data_to_transmit=ghost)], 0.102, [0])
    refused(-1, "names a cell twice", [ok(), ok()], 0.102, [0, 0])
    refused(-1, "mixed call", [ok(), ok(hol_delay=np.zeros(U))], 0.102, [0, 1])
    refused(-1, "CQI 0 outside", [dict(n_users=0), ok(cqi=np.zeros((U, R_SMALL), np.uint8))], 0.102, [0, 1])
    # a NULL data_to_transmit[k] with users: below the Python layer, which always passes one
    import ctypes as C
    tin, tout, _res, keep = rs.api._marshal_tti(3, R_SMALL, G_SMALL, 9, synth_cqi(97, (U, R_SMALL), HIST), None)
    t, ids, data = np.array([0.102]), np.array([0], np.int32), (C.POINTER(C.c_int32) * 1)()
    rc = rs.lib().rs_group_schedule_tti_queued(g._h, 1, ids.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(tin), C.byref(tout),
                                               t.ctypes.data_as(C.POINTER(C.c_double)), data)
    assert rc == -1 and "is NULL" in rs.lib().rs_last_error().decode() and whole_state(g) == state
    # ... and the accepted call still works afterwards
    g.schedule_tti_queued([ok(), dict(n_users=0)], 0.102, cell_ids=[1, 0])
    assert whole_state(g) != state
    g.close()


# ---- 9. coexistence ----

@pytest.mark.gpu
def test_plain_calls_subsets_and_switching_forms(rs, oracle):
    sched, U = 9, sum(UES)
    run = oracle_run(oracle, sched)
    g = make_group(rs, sched)
    rng = np.random.default_rng(9)
    S = g.slices.n_slices
    for k in range(CELLS):
        g.set_bearers(k, run["kinds"][k] != 0, np.full((U, 2), 100000.0), 0.1)
    # the oracle's record served cell by cell in changing order and in subsets; plain calls in between touch no bearer state
    for t, row in enumerate(run["steps"][:30]):
        order = [int(x) for x in rng.permutation(CELLS)]
        parts = [order] if t % 3 == 0 else [order[:1], order[1:]]
        calls = device_calls(sched, row)
        for part in parts:
            res = g.schedule_tti_queued([calls[k] for k in part], run["ticks"][t], cell_ids=part)
            for r, k in zip(res, part):
                same_as_oracle(r, row[k], S, g.R, f"TTI {t} cell {k} (order {order})")
            if t % 5 == 0:
                bearers = [g.get_bearers(k) for k in range(CELLS)]
                offs = [g.slice_offset(k) for k in range(CELLS)]
                g.schedule_tti([dict(cqi=synth_cqi(900 + t, (U, R_SMALL), HIST), avg_rate=rng.uniform(1e3, 5e6, U))] * CELLS)
                for k in range(CELLS):
                    got = g.get_bearers(k)
                    assert BITS(got[0]) == BITS(bearers[k][0]) and BITS(got[1]) == BITS(bearers[k][1]) and got[2] == bearers[k][2]
                    g.set_slice_offset(k, offs[k])  # (the plain call moved the slice state: the oracle did not take part)
    # cell 0: bearers -> averages -> bearers; each time it behaves as a fresh cell of that form
    fresh = make_group(rs, sched)
    a0 = rng.uniform(1e3, 5e6, U)
    call = dict(cqi=synth_cqi(990, (U, R_SMALL), HIST), rand0=5, rand1=6)
    for grp in (g, fresh):
        grp.set_avg(0, a0, 0.2)
    with pytest.raises(rs.RadioSaberError, match="not bearer-resident"):
        g.get_bearers(0)
    with pytest.raises(rs.RadioSaberError, match="not bearer-resident"):
        g.schedule_tti_queued([dict(n_users=0)], 0.201, cell_ids=[0])
    fresh.set_slice_offset(0, g.slice_offset(0))
    for now in (0.201, 0.202):
        r, w = g.schedule_tti_at([call], now, cell_ids=[0])[0], fresh.schedule_tti_at([call], now, cell_ids=[0])[0]
        assert all(BITS(getattr(r, f)) == BITS(getattr(w, f)) for f in FIELDS)
        assert all(BITS(x) == BITS(y) for x, y in zip(g.get_avg(0)[:2], fresh.get_avg(0)[:2]))
    has = np.ones((U, 2), bool)
    qcall = dict(call, data_to_transmit=np.tile(np.array([300, 900], np.int32), (U, 1)))
    for grp in (g, fresh):
        grp.set_bearers(0, has, np.stack([a0, a0[::-1]], axis=1), 0.3)
    with pytest.raises(rs.RadioSaberError, match="not resident"):
        g.get_avg(0)
    for now in (0.301, 0.302):
        r, w = g.schedule_tti_queued([qcall], now, cell_ids=[0])[0], fresh.schedule_tti_queued([qcall], now, cell_ids=[0])[0]
        assert all(BITS(getattr(r, f)) == BITS(getattr(w, f)) for f in FIELDS)
        assert all(BITS(x) == BITS(y) for x, y in zip(g.get_bearers(0)[:2], fresh.get_bearers(0)[:2]))
    assert g.get_bearers(0)[1].any()
    g.close()
    fresh.close()


# ---- 10. after specialize() and specialize_resident() ----

@pytest.mark.gpu
def test_run_time_builds_do_not_reach_queued_calls(rs, oracle):
    run = oracle_run(oracle, 9)
    plain, built = [], []
    g = make_group(rs, 9)
    follow_the_oracle(g, run, 9, "built-in", collect=plain)
    g.close()
    g = make_group(rs, 9)
    g.specialize()
    g.specialize_resident()
    assert g.jit_status()[0] == 1 and g.resident_jit_status()[0] == 1
    follow_the_oracle(g, run, 9, "after specialize", collect=built)
    assert g.kernel_name.startswith("rs_group_queued_kernel<9,")
    assert plain == built
    U = sum(UES)
    g.schedule_tti([dict(cqi=synth_cqi(1, (U, R_SMALL), HIST), avg_rate=np.full(U, 1e5))] * CELLS)
    assert g.kernel_name == "rs_group_kernel_jit"
    g.close()
