"""Counted bearers of a group's cells (rs_group_set_counters / rs_group_get_counters / rs_group_schedule_tti_counted): a queued call
that also keeps RadioBearer's m_cumulateBytes / m_cumulateRBs of both bearers of every user on the device and returns, per call
position and bearer, the bytes DoStopSchedule's loop sent.

Checked against the oracle's DoSchedule() with queues (rso_cell_step_queues and the counters of rso_cell_get_bearer_state: UNPINNED,
tests/PINS.md -- these tests prove device == oracle) and against the queued call on a twin group.  Every comparison is bitwise.  The
scenario and the proof that it binds (split grants, finite credits, data-less bearers, idle cells, RB counters that differ between a
user's bearers) are tests/test_group_counted_abi.py's.

On the parent every test of this file fails (GroupScheduler has no set_counters / schedule_tti_counted, the library
no rs_group_*_counters symbol)."""
import numpy as np
import pytest

from conftest import synth_cqi
from test_group_counted_abi import SCHEDS, counted_run
from test_group_queued_abi import CELLS, FIELDS, G_SMALL, HIST, PER_USER, R_SMALL, UES, credit

BITS = lambda a: np.ascontiguousarray(a).tobytes()  # noqa: E731


def make_group(rs, sched, ues=UES, R=R_SMALL, G=G_SMALL, K=CELLS, **cfg):
    return rs.GroupScheduler(rs.SliceConfig(ues, **cfg), R, G, K, sched=sched)


def device_calls(sched, row):
    """One TTI's records of counted_run as the calls of schedule_tti_counted / _queued: the active users, or an update-only slot."""
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


def same_as_oracle(res, st, what):
    out, ids = st["out"], st["ids"]
    for f in FIELDS:
        want = getattr(out, f)
        np.testing.assert_array_equal(getattr(res, f), want[ids] if f in PER_USER else want, err_msg=f"{what}: {f}")
    want = np.array([credit(out.user_tbs_bits[u], st["data"][i]) for i, u in enumerate(ids)], np.int32).reshape(-1, 2)
    assert res.sent.dtype == np.int32 and res.sent.shape == (len(ids), 2), f"{what}: shape of .sent"
    np.testing.assert_array_equal(res.sent, want, err_msg=f"{what}: sent")


def start(g, run, counters=True):
    K, U = len(run["kinds"]), len(run["kinds"][0])
    for k in range(K):
        g.set_bearers(k, run["kinds"][k] != 0, np.full((U, 2), 100000.0), 0.1)
        if counters:
            g.set_counters(k)


def counters_as_the_oracle(g, run, t1, what):
    for k, kd in enumerate(run["kinds"]):
        has = kd != 0
        cb, cr = g.get_counters(k)
        assert cb.dtype == np.int64 and cr.dtype == np.int64
        np.testing.assert_array_equal(cb[has], run["cum_bytes"][t1][k][has], err_msg=f"{what}: cum_bytes of cell {k} after TTI {t1}")
        np.testing.assert_array_equal(cr[has], run["cum_rbs"][t1][k][has], err_msg=f"{what}: cum_rbs of cell {k} after TTI {t1}")
        assert not cb[~has].any() and not cr[~has].any(), f"{what}: a bearer that does not exist was counted"
        avg, _, last = g.get_bearers(k)
        assert BITS(avg[has]) == BITS(run["state"][t1][k][has]), f"{what}: averages of cell {k} after TTI {t1}"
        assert not avg[~has].any() and last == run["ticks"][t1 - 1]


def follow_the_oracle(g, run, sched, what, collect=None):
    start(g, run)
    for t, row in enumerate(run["steps"]):
        res = g.schedule_tti_counted(device_calls(sched, row), run["ticks"][t])
        for k, r in enumerate(res):
            same_as_oracle(r, row[k], f"{what} TTI {t} cell {k}")
            if collect is not None:
                collect.append(b"".join(BITS(getattr(r, f)) for f in FIELDS) + BITS(r.sent))
        if t + 1 in run["state"]:
            counters_as_the_oracle(g, run, t + 1, what)
            if collect is not None:
                collect += [BITS(x) for k in range(len(res)) for x in g.get_counters(k)]


# ---- 1. against the oracle's DoSchedule() with queues ----

@pytest.mark.gpu
@pytest.mark.parametrize("sched", SCHEDS)
def test_counted_calls_against_the_oracle(rs, oracle, sched):
    run = counted_run(oracle, sched)
    g = make_group(rs, sched)
    follow_the_oracle(g, run, sched, f"sched {sched}")
    assert g.kernel_name.startswith(f"rs_group_counted_kernel<{sched},")
    g.close()


# ---- 2. a counted call is a queued call ----

@pytest.mark.gpu
@pytest.mark.parametrize("sched", [9, 7])
def test_counted_equals_queued(rs, oracle, sched):
    run = counted_run(oracle, sched)
    g, twin = make_group(rs, sched), make_group(rs, sched)
    start(g, run)
    start(twin, run, counters=False)
    for t, row in enumerate(run["steps"]):
        calls = device_calls(sched, row)
        res, want = g.schedule_tti_counted(calls, run["ticks"][t]), twin.schedule_tti_queued(calls, run["ticks"][t])
        for k in range(CELLS):
            for f in FIELDS:
                np.testing.assert_array_equal(getattr(res[k], f), getattr(want[k], f), err_msg=f"sched {sched} TTI {t} cell {k}: {f}")
            assert want[k].sent is None
            (a, p, l), (ta, tp, tl) = g.get_bearers(k), twin.get_bearers(k)
            assert BITS(a) == BITS(ta) and BITS(p) == BITS(tp) and l == tl, f"sched {sched} TTI {t} cell {k}: bearer stores"
            assert BITS(g.slice_offset(k)) == BITS(twin.slice_offset(k)), f"sched {sched} TTI {t} cell {k}: slice state"
    assert g.launch_count == twin.launch_count and g.image_stats == twin.image_stats
    g.close()
    twin.close()


# ---- 3. more call positions than threads ----

@pytest.mark.gpu
def test_more_positions_than_threads(rs, oracle):
    """2 x 350 users: up to 700 call positions on 512 threads -- the rows and the counters of the positions from the 513th on are
    written by the per-position loop's second pass."""
    kw = dict(ues=[350, 350], R=4, G=2, K=2)
    run = counted_run(oracle, 9, n_tti=12, grid_every=5, seed=3, busy=0.5, state_at=(1, 2, 12), **kw)
    assert max(len(st["ids"]) for row in run["steps"] for st in row) > 512
    g = make_group(rs, 9, **kw)
    start(g, run)
    beyond = 0
    for t, row in enumerate(run["steps"]):
        res = g.schedule_tti_counted(device_calls(9, row), run["ticks"][t])
        for k, r in enumerate(res):
            same_as_oracle(r, row[k], f"700 users TTI {t} cell {k}")  # (every row, the zero rows of the positions without a grant too)
            beyond += int((r.sent[512:] > 0).any(axis=1).sum())
        if t + 1 in run["state"]:
            counters_as_the_oracle(g, run, t + 1, "700 users")
    assert beyond > 0, "no position past the 512th was credited"
    g.close()


# ---- 4. update-only slots ----

def simple_call(rng, seed, n, data=None):
    return dict(cqi=synth_cqi(seed, (n, R_SMALL), HIST), rand0=int(rng.integers(0, 2**31 - 1)), rand1=int(rng.integers(0, 2**31 - 1)),
                data_to_transmit=np.tile(np.array([700, 0], np.int32), (n, 1)) if data is None else data)


def all_counters(g, cells=range(CELLS)):
    return b"".join(BITS(x) for k in cells for x in g.get_counters(k))


@pytest.mark.gpu
def test_update_only_slots_move_no_counter(rs):
    U = sum(UES)
    g = make_group(rs, 9)
    rng = np.random.default_rng(7)
    has = np.ones((U, 2), bool)
    for k in range(CELLS):
        g.set_bearers(k, has, np.full((U, 2), 2e5), 0.1)
        g.set_counters(k)
    res = g.schedule_tti_counted([simple_call(rng, 70 + k, U) for k in range(CELLS)], 0.101)
    assert all(r.sent.any() for r in res)
    before = [g.get_counters(k) for k in range(CELLS)]
    assert all(b[0].any() and b[1].any() for b in before)
    # a mixed call: cell 1 has nobody to schedule
    launches = g.launch_count
    res = g.schedule_tti_counted([simple_call(rng, 80, U), dict(n_users=0), simple_call(rng, 82, U)], 0.102)
    assert res[1].sent.shape == (0, 2) and (res[1].rbg_to_user == -1).all()
    assert g.launch_count == launches + 1
    after = [g.get_counters(k) for k in range(CELLS)]
    assert BITS(after[1][0]) == BITS(before[1][0]) and BITS(after[1][1]) == BITS(before[1][1])
    for k in (0, 2):  # ... while its neighbours' counters moved by what the call sent and by the PRBs of the credited positions
        np.testing.assert_array_equal(after[k][0] - before[k][0], res[k].sent)
        np.testing.assert_array_equal(after[k][1] - before[k][1], np.where(res[k].sent > 0, res[k].user_nprb[:, None], 0))
    assert g.get_bearers(1)[2] == 0.102 and not g.get_bearers(1)[1].any()  # (the update itself was done)
    # all slots empty, named out of order: still one launch, no counter moves
    state, launches = all_counters(g), g.launch_count
    res = g.schedule_tti_counted([dict(n_users=0)] * CELLS, [0.103, 0.104, 0.105], cell_ids=[2, 0, 1])
    assert g.launch_count == launches + 1 and all(r.sent.shape == (0, 2) for r in res)
    assert [g.get_bearers(k)[2] for k in range(CELLS)] == [0.104, 0.105, 0.103]
    assert all_counters(g) == state
    # the same clock again
    g.schedule_tti_counted([dict(n_users=0)], [0.104], cell_ids=[0])
    assert all_counters(g) == state
    g.close()


# ---- 5. 64-bit counters ----

@pytest.mark.gpu
def test_the_carry_into_the_upper_word(rs):
    U = sum(UES)
    g = make_group(rs, 9)
    rng = np.random.default_rng(5)
    has = np.ones((U, 2), bool)
    g.set_bearers(0, has, np.full((U, 2), 2e5), 0.1)
    cb0, cr0 = np.zeros((U, 2), np.int64), np.zeros((U, 2), np.int64)
    cb0[:], cr0[:] = 2**32 - 10, 2**32 - 1  # (whichever bearers the call credits: more than 10 bytes and more than 1 PRB carry over)
    cb0[1], cr0[1] = 0, 0
    cb0[5, 1], cr0[5, 0] = 2**40 + 3, 2**62
    g.set_counters(0, cb0, cr0)
    got = g.get_counters(0)
    assert BITS(got[0]) == BITS(cb0) and BITS(got[1]) == BITS(cr0)
    data = np.tile(np.array([300, 900], np.int32), (U, 1))
    res = g.schedule_tti_counted([simple_call(rng, 50, U, data)], 0.101, cell_ids=[0])[0]
    add_b = res.sent.astype(np.int64)
    add_r = np.where(res.sent > 0, res.user_nprb[:, None], 0).astype(np.int64)
    low = cb0 == 2**32 - 10
    assert (add_b[low] > 10).any() and (add_r[cr0 == 2**32 - 1] > 1).any(), "no bearer started below 2^32 and was carried over it"
    cb, cr = g.get_counters(0)
    np.testing.assert_array_equal(cb, cb0 + add_b)
    np.testing.assert_array_equal(cr, cr0 + add_r)
    assert (cb >= 2**32).any() and (cr >= 2**32).any()
    g.set_counters(0, None, None)
    assert not any(x.any() for x in g.get_counters(0))
    for bad in ((cb0 - 2**33, None), (None, -cr0)):
        with pytest.raises(rs.RadioSaberError, match="negative") as e:
            g.set_counters(0, *bad)
        assert e.value.code == -1
    assert not any(x.any() for x in g.get_counters(0))
    g.close()


# ---- 6. rules ----

def whole_state(g, cells=range(CELLS)):
    """everything a rejected call must leave alone, as bytes"""
    parts = []
    for k in cells:
        a, p, l = g.get_bearers(k)
        parts += [BITS(g.slice_offset(k)), BITS(a), BITS(p), np.float64(l).tobytes()]
        try:
            parts += [BITS(x) for x in g.get_counters(k)]
        except Exception:
            parts.append(b"not counted")
    return b"".join(parts) + repr((g.launch_count, g.image_stats)).encode()


@pytest.mark.gpu
def test_counted_call_rules(rs):
    U = sum(UES)
    g = make_group(rs, 9)
    rng = np.random.default_rng(8)
    has = np.ones((U, 2), bool)
    has[2, 1] = False
    for k in range(CELLS):
        g.set_bearers(k, has, np.full((U, 2), 3e5 + k), 0.1)
    with pytest.raises(rs.RadioSaberError, match="cell 1 is not counted") as e:
        g.get_counters(1)
    assert e.value.code == -4
    g.set_counters(0)
    g.set_counters(2)
    ok = lambda seed=99, **kw: dict(simple_call(rng, seed, U), cqi_epoch=3, **kw)  # noqa: E731
    g.schedule_tti_counted([ok(90), ok(91)], 0.101, cell_ids=[0, 2])
    state = whole_state(g)

    def refused(code, match, calls, now, ids):
        with pytest.raises(rs.RadioSaberError, match=match) as e:
            g.schedule_tti_counted(calls, now, cell_ids=ids)
        assert e.value.code == code, e.value
        assert whole_state(g) == state, f"a rejected call moved something ({match})"

    refused(-4, "cell 1 is not counted", [ok(), ok()], 0.102, [0, 1])
    # a bad data word in the LAST slot: the slots before it were already packed
    neg = np.tile(np.array([700, 0], np.int32), (U, 1))
    neg[U - 1, 0] = -1
    refused(-1, "negative", [ok(), ok(data_to_transmit=neg)], 0.102, [0, 2])
    ghost = np.tile(np.array([700, 0], np.int32), (U, 1))
    ghost[2, 1] = 10
    refused(-1, "has no bearer of priority 1", [ok(), ok(data_to_transmit=ghost)], 0.102, [2, 0])
    # a cell that is not bearer-resident
    g.set_avg(1, np.full(U, 5e5), 0.1)
    state = whole_state(g, cells=(0, 2))
    with pytest.raises(rs.RadioSaberError, match="cell 1 is not bearer-resident") as e:
        g.schedule_tti_counted([ok()], 0.102, cell_ids=[1])
    assert e.value.code == -4
    with pytest.raises(rs.RadioSaberError, match="cell 1 is not bearer-resident") as e:
        g.set_counters(1)
    assert e.value.code == -4 and whole_state(g, cells=(0, 2)) == state
    # queued and plain calls on a counted cell leave the counters alone
    before = all_counters(g, (0, 2))
    res = g.schedule_tti_queued([ok(92), ok(93)], 0.102, cell_ids=[0, 2])
    assert all(r.user_tbs_bits.any() and r.sent is None for r in res) and g.kernel_name.startswith("rs_group_queued_kernel<9,")
    g.schedule_tti([dict(cqi=synth_cqi(94, (U, R_SMALL), HIST), avg_rate=np.full(U, 1e5))] * 2, cell_ids=[0, 2])
    assert all_counters(g, (0, 2)) == before
    # set_bearers keeps the counters and the counted state
    g.set_bearers(0, has, np.full((U, 2), 4e5), 0.2)
    assert all_counters(g, (0,)) == before[:len(before) // 2]
    both = np.tile(np.array([300, 900], np.int32), (U, 1))
    both[2, 1] = 0
    res = g.schedule_tti_counted([ok(95, data_to_transmit=both)], 0.201, cell_ids=[0])[0]
    assert res.sent[:, 1].any() and not res.sent[2, 1] and g.kernel_name.startswith("rs_group_counted_kernel<9,")
    cb, cr = g.get_counters(0)
    assert not cb[2, 1] and not cr[2, 1], "a bearer that does not exist was written"
    # set_avg ends the counted state; set_bearers alone does not bring it back
    g.set_avg(0, np.full(U, 5e5), 0.3)
    with pytest.raises(rs.RadioSaberError, match="not counted"):
        g.get_counters(0)
    g.set_bearers(0, has, np.full((U, 2), 4e5), 0.3)
    with pytest.raises(rs.RadioSaberError, match="cell 0 is not counted"):
        g.schedule_tti_counted([ok()], 0.301, cell_ids=[0])
    g.set_counters(0)
    assert not any(x.any() for x in g.get_counters(0))
    g.close()


@pytest.mark.gpu
def test_queued_builds_do_not_reach_counted_calls(rs, oracle):
    run = counted_run(oracle, 9, n_tti=40, state_at=(1, 2, 40))
    built_in, built = [], []
    g = make_group(rs, 9)
    follow_the_oracle(g, run, 9, "built-in", collect=built_in)
    g.close()
    g = make_group(rs, 9)
    g.specialize_queued()
    status = g.queued_jit_status()
    assert status[0] == 1
    follow_the_oracle(g, run, 9, "after specialize_queued", collect=built)
    assert g.kernel_name.startswith("rs_group_counted_kernel<9,")
    assert built == built_in
    assert g.queued_jit_status() == status
    g.close()


# ---- 7. the reference's log lines ----

@pytest.mark.gpu
def test_the_app_lines_of_a_counted_run(rs, oracle):
    from radiosaber_amd import logfmt
    sched, n_tti, U = 8, 40, sum(UES)
    run = counted_run(oracle, sched, n_tti=n_tti, state_at=(n_tti,))
    g = make_group(rs, sched)
    start(g, run)
    apps = logfmt.app_ids(rs.SliceConfig(UES, traffic=[{"internet_flow": 2}] * len(UES)))  # two applications per UE: ids 2u, 2u + 1
    u2s = np.asarray(g.slices.user_to_slice)
    lines = [[] for _ in range(CELLS)]
    tracked = [(np.zeros((U, 2), np.int64), np.zeros((U, 2), np.int64)) for _ in range(CELLS)]
    for t, row in enumerate(run["steps"]):
        res = g.schedule_tti_counted(device_calls(sched, row), run["ticks"][t])
        for k, r in enumerate(res):
            ids = row[k]["ids"]
            # the counters tracked from .sent and user_nprb; every other TTI read back as well: the same numbers
            cb, cr = tracked[k]
            cb[ids] += r.sent
            cr[ids] += np.where(r.sent > 0, r.user_nprb[:, None], 0)
            if t % 2:
                got = g.get_counters(k)
                assert BITS(got[0]) == BITS(cb) and BITS(got[1]) == BITS(cr)
            new = logfmt.counted_call_lines(100 + t, ids, r.sent, None, cb, cr, apps, u2s)
            assert len(new) == int((r.sent > 0).sum())
            lines[k] += new
    for k in range(CELLS):
        assert lines[k], f"cell {k} printed nothing"
        mbps, rbs = logfmt.slice_throughput_from_log(lines[k], 2 * U, len(UES), begin_ts=0, end_ts=1000)  # (one second: bytes * 8 / 1e6)
        for s in range(len(UES)):
            assert round(mbps[s] * 1e6 / 8) == int(run["cum_bytes"][n_tti][k][u2s == s].sum()), f"cell {k} slice {s}: bytes"
            assert round(rbs[s]) == int(run["cum_rbs"][n_tti][k][u2s == s].sum()), f"cell {k} slice {s}: RBs"
    g.close()
