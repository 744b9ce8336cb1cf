"""Resident flows of a scheduler-1 group's cells (rs_group_set_flows / rs_group_schedule_tti_flows): the device keeps both bearers of
every user -- average, bytes credited since the last update, existence, m_cumulateBytes, m_cumulateRBs --, applies the reference's
EWMA to every existing bearer, races the call's FLOWS (a position is one bearer of one user) on their own averages with the
data_to_transmit gate and credits the whole transport block to the flow.

Checked against the oracle's DoSchedule() with queues (rso_cell_step_queues -> step_pf_flows: UNPINNED, tests/PINS.md -- these tests
prove device == oracle) and against the resident-averages call in the case where both forms must agree.  Every comparison is
bitwise.  The scenario and the proof that it binds are tests/test_group_flows_abi.py's."""
import ctypes as C

import numpy as np
import pytest

from conftest import synth_cqi
from test_group_flows_abi import AVG0, LAST0, SCHED_PF, USERS, flows_run
from test_group_queued_abi import CELLS, G_SMALL, HIST, INFINITE, R_SMALL

BITS = lambda a: np.ascontiguousarray(a).tobytes()  # noqa: E731
FIELDS = ("target_rbs", "quota_rbgs", "rbg_to_user", "user_nprb", "user_final_cqi", "user_mcs", "user_tbs_bits")


def make_group(rs, n_users=2 * USERS, R=R_SMALL, G=G_SMALL, K=CELLS, sched=SCHED_PF):
    """one slice; n_users is the group's capacity of call positions (the largest flow count) and of user ids"""
    return rs.GroupScheduler(rs.SliceConfig([n_users]), R, G, K, sched=sched)


def pad(a, rows):
    out = np.zeros((rows,) + a.shape[1:], a.dtype)
    out[:len(a)] = a
    return out


def flows_call(st, epoch=None, prb=0):
    """one record of flows_run as a call of schedule_tti_flows: the flows with data, or an update-only slot"""
    if len(st["uid"]) == 0:
        return dict(n_users=0)
    kw = dict(user_id=st["uid"], flow_bearer=st["fb"], data_to_transmit=st["data"], cqi_epoch=st["epoch"] if epoch is None else epoch)
    if prb:
        kw["cqi_prb"] = np.repeat(st["cqi"], prb, axis=1)  # every PRB of an RBG reports the RBG's value: the oracle's grid
    else:
        kw["cqi"] = st["cqi"]
    return kw


def same_as_oracle(res, st, what):
    """rbg_to_user as flow ids; per user the sums over its positions; final CQI and MCS of the user's last position with PRBs"""
    out, uid = st["out"], st["uid"]
    U = len(out.user_nprb)
    np.testing.assert_array_equal(res.rbg_to_user, out.rbg_to_user, err_msg=f"{what}: rbg_to_user (flow ids)")
    nprb, tbs = np.zeros(U, np.int64), np.zeros(U, np.int64)
    np.add.at(nprb, uid, res.user_nprb)
    np.add.at(tbs, uid, res.user_tbs_bits)
    np.testing.assert_array_equal(nprb, out.user_nprb, err_msg=f"{what}: user_nprb summed per user")
    np.testing.assert_array_equal(tbs, out.user_tbs_bits, err_msg=f"{what}: user_tbs_bits summed per user")
    fcqi, mcs = np.zeros(U, np.int64), np.zeros(U, np.int64)
    for i, u in enumerate(uid):  # ascending positions: the last one with PRBs stays
        if res.user_nprb[i] > 0:
            fcqi[u], mcs[u] = res.user_final_cqi[i], res.user_mcs[i]
    np.testing.assert_array_equal(fcqi, out.user_final_cqi, err_msg=f"{what}: final CQI of the user's last flow with PRBs")
    np.testing.assert_array_equal(mcs, out.user_mcs, err_msg=f"{what}: MCS of the user's last flow with PRBs")
    assert len(res.user_tbs_bits) == len(uid)


def set_all_flows(g, run):
    cap = g.slices.n_users
    for k, kd in enumerate(run["kinds"]):
        g.set_flows(k, pad(kd != 0, cap), np.full((cap, 2), AVG0), LAST0)


def same_state(g, run, t, res, row, what):
    """averages, counters and pending bytes of every bearer after TTI t + 1 (counted from 1)"""
    for k, st in enumerate(row):
        U = len(run["kinds"][k])
        a, p, last, cb, cr = g.get_flows(k)
        has = run["kinds"][k] != 0
        assert BITS(a[:U][has]) == BITS(run["state"][t + 1][k][has]), f"{what}: averages of cell {k} after TTI {t + 1}"
        assert not a[:U][~has].any() and not a[U:].any(), f"{what}: a bearer that does not exist reports an average"
        np.testing.assert_array_equal(cb[:U], run["cum_bytes"][t + 1][k], err_msg=f"{what}: cum_bytes of cell {k} after TTI {t + 1}")
        np.testing.assert_array_equal(cr[:U], run["cum_rbs"][t + 1][k], err_msg=f"{what}: cum_rbs of cell {k} after TTI {t + 1}")
        assert not cb[U:].any() and not cr[U:].any()
        want = np.zeros_like(p)  # the update of this TTI emptied them, then the call credited its positions
        want[st["uid"], st["fb"]] = res[k].user_tbs_bits // 8
        np.testing.assert_array_equal(p, want, err_msg=f"{what}: pending bytes of cell {k} after TTI {t + 1}")
        assert last == run["ticks"][t]


def flows_bits(g, k):
    """a flow-resident cell's whole state as bytes"""
    return b"".join(np.float64(x).tobytes() if isinstance(x, float) else BITS(x) for x in g.get_flows(k))


def follow_the_oracle(g, run, what):
    set_all_flows(g, run)
    for t, row in enumerate(run["steps"]):
        res = g.schedule_tti_flows([flows_call(st) for st in row], run["ticks"][t])
        for k, st in enumerate(row):
            same_as_oracle(res[k], st, f"{what} TTI {t} cell {k}")
        if t + 1 in run["state"]:
            same_state(g, run, t, res, row, what)


# ---- 1. against the oracle over the scenario, every TTI ----

@pytest.mark.gpu
def test_flows_calls_against_the_oracle(rs, oracle):
    run = flows_run(oracle)
    g = make_group(rs)
    follow_the_oracle(g, run, "flows")
    assert g.kernel_name == "rs_group_flows_kernel<1, 0>"
    assert g.launch_count == len(run["steps"])
    g.close()


# ---- 2. more flows than threads ----

@pytest.mark.gpu
def test_more_flows_than_threads(rs, oracle):
    """2 cells x 350 users with two bearers: the gather and the credit stride over more than 512 call positions, the update over
    2 048 bearers.  The group holds 1 024 positions, RS_MAX_USERS: the library refuses a config with more (the 1 400 first meant
    for this case -- both cells' bearers together -- cannot be created), and a cell lists 700 flows at the most."""
    run = flows_run(oracle, users=350, R=4, G=2, K=2, n_tti=12, grid_every=5, seed=3, busy=0.5, state_at=(1, 2, 12))
    assert max(len(st["uid"]) for row in run["steps"] for st in row) > 512
    with pytest.raises(rs.RadioSaberError, match="n_users"):
        make_group(rs, n_users=1400, R=4, G=2, K=2)
    g = make_group(rs, n_users=1024, R=4, G=2, K=2)
    follow_the_oracle(g, run, "700 flows")
    g.close()


# ---- 3. update-only slots, subsets and permutations, cqi_epoch modes mixed in one launch ----

@pytest.mark.gpu
@pytest.mark.parametrize("staged_prb", [False, True])
def test_subsets_permutations_and_image_modes(rs, oracle, monkeypatch, staged_prb):
    """The oracle's record served in changing order and in subsets.  Cell 1 promises nothing (cqi_epoch 0, mode 0), cells 0 and 2
    number their reports: mode 1 when the number, the position count or the user list changed, mode 2 otherwise.  staged_prb: per-PRB
    reports and the staged-copy path (RS_DROPIN_COPY=1) instead of per-RBG reports read in place."""
    if staged_prb:
        monkeypatch.setenv("RS_DROPIN_COPY", "1")
    run = flows_run(oracle)
    g = make_group(rs)
    set_all_flows(g, run)
    rng = np.random.default_rng(31)
    image = [None] * CELLS  # the test's mirror of the cells' image records: (epoch, user list) of the last stored call
    want = [0, 0, 0]        # reused, stored, without a promise
    launches = idle = mixed = 0
    for t, row in enumerate(run["steps"][:40]):
        order = [int(x) for x in rng.permutation(CELLS)]
        parts = [order] if t % 3 == 0 else [order[:1], order[1:]]
        for part in parts:
            others = [k for k in range(CELLS) if k not in part]
            before = [flows_bits(g, k) for k in others]
            calls, modes = [], set()
            for k in part:
                st = row[k]
                epoch = 0 if k == 1 else st["epoch"]
                calls.append(flows_call(st, epoch=epoch, prb=G_SMALL if staged_prb else 0))
                if len(st["uid"]) == 0:
                    idle += 1
                    continue
                key = (epoch, BITS(st["uid"]))
                mode = 0 if epoch == 0 else (2 if image[k] == key else 1)
                want[{2: 0, 1: 1, 0: 2}[mode]] += 1
                image[k] = key if mode else None
                modes.add(mode)
            mixed += len(modes) == 3
            res = g.schedule_tti_flows(calls, run["ticks"][t], cell_ids=part)
            launches += 1
            for r, k in zip(res, part):
                same_as_oracle(r, row[k], f"TTI {t} cell {k} (order {order})")
                if len(row[k]["uid"]) == 0:
                    assert (r.rbg_to_user == -1).all() and not r.target_rbs.any() and not r.quota_rbgs.any()
            after = [flows_bits(g, k) for k in others]
            assert before == after, f"TTI {t}: a cell the call did not name moved"
        if t + 1 in run["state"]:
            full = g.schedule_tti_flows([dict(n_users=0)] * CELLS, run["ticks"][t])  # (the same clock: nothing moves)
            launches += 1
            for k in range(CELLS):
                a, _, last, cb, cr = g.get_flows(k)
                U, has = USERS, run["kinds"][k] != 0
                assert BITS(a[:U][has]) == BITS(run["state"][t + 1][k][has]) and last == run["ticks"][t]
                np.testing.assert_array_equal(cb[:U], run["cum_bytes"][t + 1][k])
                np.testing.assert_array_equal(cr[:U], run["cum_rbs"][t + 1][k])
            assert all((r.rbg_to_user == -1).all() for r in full)
    assert idle > 0 and mixed > 0 and all(w > 0 for w in want), (idle, mixed, want)
    assert g.image_stats == tuple(want) and g.launch_count == launches
    g.close()


# ---- 4. one InfiniteBuffer bearer per user, ids 0..n-1: the resident-averages call of a twin group ----

@pytest.mark.gpu
def test_one_infinite_bearer_per_user_equals_the_resident_call(rs):
    K, U = CELLS, USERS
    g, twin = make_group(rs, n_users=U), make_group(rs, n_users=U)
    rng = np.random.default_rng(67)
    has = np.zeros((U, 2), bool)
    has[:, 0] = True
    for k in range(K):
        a0 = rng.uniform(1e3, 5e6, U)
        g.set_flows(k, has, np.stack([a0, np.zeros(U)], axis=1), 0.1)
        twin.set_avg(k, a0, 0.1)
    served = np.zeros((K, U), np.int64)
    for t in range(40):
        now = 0.1 + 0.001 * (t + 1)
        calls = [dict(cqi=synth_cqi(6100 + 10 * t + k, (U, R_SMALL), HIST), cqi_epoch=1 + t // 10) for k in range(K)]
        res = g.schedule_tti_flows([dict(c, flow_bearer=np.zeros(U, np.uint8), data_to_transmit=np.full(U, INFINITE, np.int32)) for c in calls], now)
        want = twin.schedule_tti_at(calls, now)
        for k in range(K):
            for f in FIELDS:
                w = getattr(want[k], f)
                if f == "rbg_to_user":
                    w = np.where(w >= 0, 2 * w, -1)  # flow ids: bearer 0 of the user
                np.testing.assert_array_equal(getattr(res[k], f), w, err_msg=f"TTI {t} cell {k}: {f}")
            (a, p, l, cb, cr), (ta, tp, tl) = g.get_flows(k), twin.get_avg(k)
            assert BITS(a[:, 0]) == BITS(ta) and BITS(p[:, 0]) == BITS(tp) and l == tl, f"TTI {t} cell {k}: resident state"
            assert not a[:, 1].any() and not p[:, 1].any() and not cb[:, 1].any() and not cr[:, 1].any()
            served[k] += res[k].user_tbs_bits // 8
            np.testing.assert_array_equal(cb[:, 0], served[k])
    assert served.any()
    g.close()
    twin.close()


# ---- 5. refusals move nothing ----

def whole_state(g, cells=range(CELLS)):
    """everything a rejected call must leave alone, as bytes"""
    parts = []
    for k in cells:
        parts.append(BITS(g.slice_offset(k)))
        try:
            a, p, l, cb, cr = g.get_flows(k)
        except Exception:
            a, p, l = g.get_avg(k)
            cb = cr = np.zeros(0)
        parts += [BITS(a), BITS(p), np.float64(l).tobytes(), BITS(cb), BITS(cr)]
    return b"".join(parts) + repr((g.launch_count, g.image_stats)).encode()


def plain_flows_call(seed, uid, fb, data=700, **kw):
    uid = np.asarray(uid, np.int32)
    return dict(dict(cqi=synth_cqi(seed, (len(uid), R_SMALL), HIST), user_id=uid, flow_bearer=np.asarray(fb, np.uint8),
                     data_to_transmit=np.full(len(uid), data, np.int32)), **kw)


@pytest.mark.gpu
def test_refusals_move_nothing(rs):
    cap = 2 * USERS
    has, avg = np.ones((cap, 2), bool), np.full((cap, 2), 1e5)
    # the wrong scheduler, and set_bearers still refused on a scheduler-1 group
    for sched in (9, 7, 10):
        other = make_group(rs, sched=sched)
        with pytest.raises(rs.RadioSaberError, match="not served") as e:
            other.set_flows(0, has, avg, 0.1)
        assert e.value.code == -1
        other.close()
    g = make_group(rs)
    with pytest.raises(rs.RadioSaberError, match="not served"):
        g.set_bearers(0, has, avg, 0.1)
    # set_flows' own refusals
    for bad in (0.5, 2.0**51 * 1.5, np.nan, np.inf):
        a = avg.copy()
        a[4, 1] = bad
        with pytest.raises(rs.RadioSaberError, match="outside 1..2\\^51"):
            g.set_flows(0, has, a, 0.1)
        h = has.copy()
        h[4, 1] = False
        g.set_flows(0, h, a, 0.1)  # the average of a bearer that does not exist is not read
        assert g.get_flows(0)[0][4, 1] == 0
    for bad in (np.nan, np.inf):
        with pytest.raises(rs.RadioSaberError, match="finite"):
            g.set_flows(0, has, avg, bad)
    neg = np.zeros((cap, 2), np.int64)
    neg[3, 0] = -1
    with pytest.raises(rs.RadioSaberError, match="negative"):
        g.set_flows(0, has, avg, 0.1, cum_bytes=neg)
    with pytest.raises(rs.RadioSaberError, match="negative"):
        g.set_flows(0, has, avg, 0.1, cum_rbs=neg)
    # the state the refused calls must leave alone: cells 0 and 1 flow-resident and served once, cell 2 average-resident
    has[2, 1] = False
    cb0 = np.arange(2 * cap, dtype=np.int64).reshape(cap, 2)
    g.set_flows(0, has, np.full((cap, 2), 3e5), 0.1, cum_bytes=cb0, cum_rbs=cb0 + 5)
    g.set_flows(1, has, np.full((cap, 2), 4e5), 0.1)
    g.set_avg(2, np.full(cap, 5e5), 0.1)
    a, p, l, cb, cr = g.get_flows(0)
    assert BITS(cb) == BITS(cb0 * has) and BITS(cr) == BITS((cb0 + 5) * has) and not p.any() and l == 0.1  # (zeros where no bearer exists)
    uid, fb = [0, 0, 1, 2, 5], [0, 1, 1, 0, 1]
    g.schedule_tti_flows([plain_flows_call(90 + k, uid, fb) for k in range(2)], 0.101, cell_ids=[0, 1])
    g.schedule_tti_at([dict(cqi=synth_cqi(95, (cap, R_SMALL), HIST))], 0.101, cell_ids=[2])
    assert g.get_flows(0)[1].any()
    state = whole_state(g)
    ok = lambda **kw: plain_flows_call(99, uid, fb, **kw)  # noqa: E731

    def refused(code, match, calls, now, ids, fn=None):
        with pytest.raises(rs.RadioSaberError, match=match) as e:
            (fn or g.schedule_tti_flows)(calls, now, cell_ids=ids)
        assert e.value.code == code, e.value
        assert whole_state(g) == state, f"a rejected call moved something ({match})"

    refused(-1, "does not ascend", [plain_flows_call(99, [0, 0, 2, 1], [0, 1, 0, 0])], 0.102, [0])  # descending users
    refused(-1, "does not ascend", [plain_flows_call(99, [0, 1, 1], [0, 1, 0])], 0.102, [0])        # descending bearers of one user
    refused(-1, "does not ascend", [plain_flows_call(99, [0, 1, 1], [0, 1, 1])], 0.102, [0])        # a flow named twice
    refused(-1, "does not exist", [plain_flows_call(99, [0, 2, 3], [0, 1, 0])], 0.102, [0])         # data on a missing bearer
    zero = np.full(len(uid), 700, np.int32)
    zero[3] = 0
    refused(-1, "a flow without data", [ok(data_to_transmit=zero)], 0.102, [0])
    refused(-1, "neither 0 nor 1", [ok(flow_bearer=np.array([0, 1, 1, 0, 2], np.uint8))], 0.102, [0])
    refused(-1, "avg_rate must be NULL", [ok(avg_rate=np.ones(len(uid)))], 0.102, [0])
    refused(-1, "hol_delay must be NULL", [ok(hol_delay=np.zeros(len(uid)))], 0.102, [0])
    refused(-1, "out of range", [plain_flows_call(99, [0, cap], [0, 0])], 0.102, [0])
    refused(-4, "cell 2 is not flow-resident", [ok(), ok()], 0.102, [0, 2])
    refused(-1, "before the cell's last update", [ok()], 0.1005, [0])
    refused(-1, "not finite", [ok()], np.nan, [0])
    refused(-1, "names a cell twice", [ok(), ok()], 0.102, [0, 0])
    refused(-1, "CQI 0 outside", [dict(n_users=0), ok(cqi=np.zeros((len(uid), R_SMALL), np.uint8))], 0.102, [0, 1])
    # the other resident calls on a flow-resident cell
    at_call = dict(cqi=synth_cqi(96, (cap, R_SMALL), HIST))
    refused(-4, "flow-resident", [at_call], 0.102, [0], fn=g.schedule_tti_at)
    q_call = dict(at_call, data_to_transmit=np.tile(np.array([700, 0], np.int32), (cap, 1)))
    refused(-4, "resident", [q_call], 0.102, [0], fn=g.schedule_tti_queued)
    refused(-4, "resident", [q_call], 0.102, [0], fn=g.schedule_tti_counted)
    for getter in (g.get_bearers, g.get_counters, g.get_avg):
        with pytest.raises(rs.RadioSaberError) as e:
            getter(0)
        assert e.value.code == -4
    with pytest.raises(rs.RadioSaberError) as e:
        g.get_flows(2)
    assert e.value.code == -4 and whole_state(g) == state
    # a NULL flow_bearer[k] with positions: below the Python layer, which always passes one
    tin, tout, _res, keep = rs.api._marshal_tti(1, R_SMALL, G_SMALL, SCHED_PF, synth_cqi(97, (3, R_SMALL), HIST), None,
                                                data_to_transmit=np.full(3, 5, np.int32))
    t, ids, fbp = np.array([0.102]), np.array([0], np.int32), (C.POINTER(C.c_uint8) * 1)()
    rc = rs.lib().rs_group_schedule_tti_flows(g._h, 1, ids.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(tin), C.byref(tout),
                                              t.ctypes.data_as(C.POINTER(C.c_double)), fbp)
    assert rc == -1 and "is NULL" in rs.lib().rs_last_error().decode() and whole_state(g) == state
    # ... and the accepted call still works afterwards; the later of set_avg / set_flows wins
    g.schedule_tti_flows([ok(), dict(n_users=0)], 0.102, cell_ids=[1, 0])
    assert whole_state(g) != state
    g.set_avg(0, np.full(cap, 5e5), 0.2)
    with pytest.raises(rs.RadioSaberError, match="not flow-resident"):
        g.get_flows(0)
    g.set_flows(0, has, np.full((cap, 2), 3e5), 0.3)
    with pytest.raises(rs.RadioSaberError, match="not resident"):
        g.get_avg(0)
    assert not g.get_flows(0)[3].any() and g.get_flows(0)[2] == 0.3
    g.close()


# ---- 6. a plain call between flows calls ----

@pytest.mark.gpu
def test_a_plain_call_between_flows_calls(rs, oracle):
    """rs_group_schedule_tti on flow-resident cells: averages, pending bytes and counters stay, and the flows calls go on as the
    oracle's."""
    run = flows_run(oracle)
    g = make_group(rs)
    set_all_flows(g, run)
    cap = g.slices.n_users
    rng = np.random.default_rng(13)
    for t, row in enumerate(run["steps"][:40]):
        res = g.schedule_tti_flows([flows_call(st) for st in row], run["ticks"][t])
        for k, st in enumerate(row):
            same_as_oracle(res[k], st, f"TTI {t} cell {k}")
        if t % 4 == 0:
            kept = [g.get_flows(k) for k in range(CELLS)]
            offs = [g.slice_offset(k) for k in range(CELLS)]
            assert any(x[1].any() for x in kept)
            g.schedule_tti([dict(cqi=synth_cqi(900 + t, (cap, R_SMALL), HIST), avg_rate=rng.uniform(1e3, 5e6, cap),
                                 data_to_transmit=np.full(cap, 3000, np.int32))] * CELLS)
            assert g.kernel_name == "rs_group_kernel<1, 0>"
            for k in range(CELLS):
                got = g.get_flows(k)
                assert all(BITS(x) == BITS(y) for x, y in zip(got, kept[k])), f"TTI {t} cell {k}: the plain call moved resident state"
                g.set_slice_offset(k, offs[k])  # (the oracle did not take part in the plain call)
        if t + 1 in run["state"]:
            same_state(g, run, t, res, row, "with plain calls in between")
    assert g.kernel_name == "rs_group_flows_kernel<1, 0>"
    g.close()
