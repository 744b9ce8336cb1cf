"""rs_group_specialize_flows: a group's own run-time builds of scheduler 1's FLOWS kernel (entry point rs_group_flows_kernel_jit,
general and lean), checked against the built-in flows kernel on outputs AND on state -- slice state, both bearers' averages, pending
bytes, m_cumulateBytes and m_cumulateRBs of every user id, the last-update time.  Against an unspecialised twin and against the
oracle's DoSchedule() with queues on the scenario of tests/test_group_flows_abi.py, on the general build's path (per-PRB reports,
staged copies), with more positions than threads, with update-only launches, with subsets, permutations and cqi_epoch modes mixed in
one launch, beside scheduler 1's other pairs, with a build that is wrong in a counter alone, and with the self-check mark that travels
to the next process.  Every comparison is bitwise."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import synth_cqi
from test_group_flows_abi import AVG0, LAST0, SCHED_PF, STATE_AT, USERS, flows_run
from test_group_queued_abi import CELLS, G_SMALL, HIST, R_SMALL
from test_gpu_group_flows import BITS, FIELDS, flows_bits, flows_call, make_group, pad, plain_flows_call, same_as_oracle, same_state, set_all_flows

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
CAP = 2 * USERS
JIT_NAME = "rs_group_flows_kernel_jit"
BUILT_IN = "rs_group_flows_kernel<1, 0>"
REF = "the built-in flows kernel field by field, bearer stores and counters included"
VERIFIED = f"verified (8 checked calls agreed with {REF})"
_RUNS = {}


@pytest.fixture(scope="module", autouse=True)
def cache_dir(tmp_path_factory):
    """The builds of this file go to a cache directory of its own: one hiprtc run per (shape, build)."""
    mp = pytest.MonkeyPatch()
    d = tmp_path_factory.mktemp("flows_builds")
    mp.setenv("RS_JIT_CACHE_DIR", str(d))
    for k in ("RS_JIT_CACHE", "RS_JIT_EXTRA", "RS_JIT_LEAN", "RS_DROPIN_SELFCHECK_CALLS", "RS_JIT_SELFCHECK", "RS_DROPIN_COPY"):
        mp.delenv(k, raising=False)
    yield d
    mp.undo()


def _run(oracle, **kw):
    key = tuple(sorted((k, str(v)) for k, v in kw.items()))
    if key not in _RUNS:
        _RUNS[key] = flows_run(oracle, **kw)
    return _RUNS[key]


def _same_results(res, want, what):
    for f in FIELDS:
        assert BITS(getattr(res, f)) == BITS(getattr(want, f)), f"{what}: {f}"


def _same_state(g, ref, cells, what):
    for k in cells:
        for name, x, y in zip(("avg", "pending_bytes", "last_update", "cum_bytes", "cum_rbs"), g.get_flows(k), ref.get_flows(k)):
            assert (x == y if isinstance(x, float) else BITS(x) == BITS(y)), f"{what}, cell {k}: {name}"


def _both(g, ref, calls, now, cell_ids=None, what="", jit=True, state=True):
    """One flows call on the specialised group and on its unspecialised twin: outputs, slice state, served-by name, and (state) the
    flows' stores."""
    res, want = g.schedule_tti_flows(calls, now, cell_ids=cell_ids), ref.schedule_tti_flows(calls, now, cell_ids=cell_ids)
    for j in range(len(calls)):
        _same_results(res[j], want[j], f"{what} slot {j}")
    assert g.kernel_name == (JIT_NAME if jit else BUILT_IN) and ref.kernel_name == BUILT_IN, (g.kernel_name, g.flows_jit_status())
    cells = range(g.n_cells) if cell_ids is None else cell_ids
    for k in cells:
        assert BITS(g.slice_offset(k)) == BITS(ref.slice_offset(k)), f"{what}, cell {k}: slice offsets"
    if state:
        _same_state(g, ref, cells, what)
    return res


def _drive(g, ref, run, what, prb=0, n_tti=None, state_every=False):
    """flows_run's steps through both groups, the specialised one held against the oracle's record as well"""
    set_all_flows(g, run)
    set_all_flows(ref, run)
    steps = run["steps"][:n_tti]
    for t, row in enumerate(steps):
        at_state = (t + 1) in run["state"]
        res = _both(g, ref, [flows_call(st, prb=prb) for st in row], run["ticks"][t], what=f"{what} TTI {t}", state=state_every or at_state)
        for k, st in enumerate(row):
            same_as_oracle(res[k], st, f"{what} TTI {t} cell {k}")
        if at_state:
            same_state(g, run, t, res, row, what)
    return len(steps)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. equal to the built-in flows kernel and to the oracle
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("selfcheck", ["2", "0"])
def test_equal_to_the_built_in_flows_kernel_and_to_the_oracle(rs, oracle, selfcheck, monkeypatch):
    monkeypatch.setenv("RS_JIT_SELFCHECK", selfcheck)
    run = _run(oracle)
    ref, g = make_group(rs), make_group(rs)
    g.specialize_flows()
    assert g.flows_jit_status()[0] == 1, g.flows_jit_status()
    assert (g.jit_status()[0], g.resident_jit_status()[0], g.queued_jit_status()[0], g.counted_jit_status()[0]) == (0, 0, 0, 0)
    n = _drive(g, ref, run, "flows")
    assert set(run["state"]) == set(STATE_AT)
    assert g.launch_count == ref.launch_count == n == len(run["steps"])   # the twin launch of a checked call is not counted
    code, msg = g.flows_jit_status()
    assert code == 1, (code, msg)
    if selfcheck == "2":   # (per-RBG reports and the gate that every flows call carries: the lean build serves)
        assert f"lean build: {VERIFIED}" in msg and "general build: 0 checked call(s) agreed" in msg, msg
    else:
        assert "agreed" not in msg, msg
    g.close()
    ref.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the general build's path
# ---------------------------------------------------------------------------------------------------------------------------

def test_general_build_path(rs, oracle, monkeypatch):
    """Per-PRB reports on the staged-copy path (RS_DROPIN_COPY=1): the general build serves those calls, the lean one none."""
    monkeypatch.setenv("RS_JIT_SELFCHECK", "2")
    monkeypatch.setenv("RS_DROPIN_COPY", "1")
    run = _run(oracle)
    assert all(any(len(st["uid"]) for st in row) for row in run["steps"][:12])   # (no call of update-only slots only: those take the lean build)
    ref, g = make_group(rs), make_group(rs)
    g.specialize_flows()
    n = _drive(g, ref, run, "per-PRB", prb=G_SMALL, n_tti=12, state_every=True)
    code, msg = g.flows_jit_status()
    assert code == 1 and f"general build: {VERIFIED}" in msg and "lean build: 0 checked call(s) agreed" in msg, msg
    assert g.launch_count == ref.launch_count == n
    g.close()
    ref.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. more positions than threads
# ---------------------------------------------------------------------------------------------------------------------------

def test_more_flows_than_threads(rs, oracle, monkeypatch):
    """2 cells x 350 users with two bearers in a 1 024-position group (the shape of tests/test_gpu_group_flows.py): the constant-stride
    update covers 2 048 bearers, gather and credit up to 700 call positions.  With equal averages the oracle's winners are early
    positions, so two calls of the test's own come first (they are checked calls too): the flows from the 256th user on start from an
    average a thousand times smaller than the others', whatever they report they win, and a position past the 512th is credited --
    by the second pass of the constant-stride loop."""
    monkeypatch.setenv("RS_JIT_SELFCHECK", "2")
    users, cap = 350, 1024
    run = _run(oracle, users=users, R=4, G=2, K=2, n_tti=12, grid_every=5, seed=3, busy=0.5, state_at=(1, 2, 12))
    assert max(len(st["uid"]) for row in run["steps"] for st in row) > 512
    ref, g = make_group(rs, n_users=cap, R=4, G=2, K=2), make_group(rs, n_users=cap, R=4, G=2, K=2)
    g.specialize_flows()
    has = np.zeros((cap, 2), bool)
    has[:users] = True
    avg = np.full((cap, 2), 5e6)
    avg[256:] = 5e3
    uid, fb = np.repeat(np.arange(users, dtype=np.int32), 2), np.tile(np.array([0, 1], np.uint8), users)
    for grp in (g, ref):
        for k in range(2):
            grp.set_flows(k, has, avg, LAST0)
    beyond = 0
    for it in range(2):
        calls = [plain_flows_call(4000 + 10 * it + k, uid, fb, data=40 if it else 100000) for k in range(2)]
        calls = [dict(c, cqi=synth_cqi(4000 + 10 * it + k, (len(uid), 4), HIST)) for k, c in enumerate(calls)]
        res = _both(g, ref, calls, LAST0 + 0.001 * (it + 1), what=f"late winners, call {it}")
        for k, r in enumerate(res):
            late = r.user_tbs_bits[512:] // 8 > 0
            beyond += int(late.sum())
            cb = g.get_flows(k)[3]
            assert (cb[uid[512:][late], fb[512:][late]] > 0).all(), "a credited position past the 512th has no bytes counted"
    assert beyond > 0, "no position past the 512th was credited"
    for grp in (g, ref):   # (the oracle did not take part in those two calls)
        for k in range(2):
            grp.set_slice_offset(k, np.zeros(1))
    n = _drive(g, ref, run, "700 flows", state_every=True)
    assert g.kernel_name == JIT_NAME and g.launch_count == ref.launch_count == n + 2
    code, msg = g.flows_jit_status()
    assert code == 1 and f"lean build: {VERIFIED}" in msg, (code, msg)
    g.close()
    ref.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. update-only launches
# ---------------------------------------------------------------------------------------------------------------------------

def _counters(g, cells=range(CELLS)):
    return b"".join(BITS(x) for k in cells for x in g.get_flows(k)[3:])


def test_update_only_launches(rs, monkeypatch):
    monkeypatch.setenv("RS_JIT_SELFCHECK", "2")
    ref, g = make_group(rs), make_group(rs)
    g.specialize_flows()
    has = np.ones((CAP, 2), bool)
    has[3] = (True, False)
    for k in range(CELLS):
        for grp in (g, ref):
            grp.set_flows(k, has, np.full((CAP, 2), 2e5), 0.1)
    every = range(CELLS)
    uid, fb = [0, 0, 1, 2, 3, 5, 5], [0, 1, 1, 0, 0, 0, 1]
    res = _both(g, ref, [plain_flows_call(70 + k, uid, fb) for k in every], 0.101, what="full call")
    assert all(r.user_tbs_bits.any() for r in res) and all(g.get_flows(k)[1].any() for k in every)
    # a mixed call inside the checked ones: cell 1 has no flow to schedule -- none of its counters moves
    before = _counters(g, [1])
    res = _both(g, ref, [plain_flows_call(80, uid, fb), dict(n_users=0), plain_flows_call(82, uid, fb)], 0.102, what="mixed call")
    assert (res[1].rbg_to_user == -1).all() and not res[1].target_rbs.any() and (res[0].rbg_to_user >= 0).any()
    assert _counters(g, [1]) == before
    assert not g.get_flows(1)[1].any() and g.get_flows(1)[2] == 0.102
    # empty slots only, named out of order, a clock per cell: one launch, a checked call like any other, no counter moves
    before = _counters(g)
    _both(g, ref, [dict(n_users=0)] * CELLS, [0.103, 0.104, 0.105], cell_ids=[2, 0, 1], what="empty slots only")
    assert _counters(g) == before
    assert [g.get_flows(k)[2] for k in every] == [0.104, 0.105, 0.103]
    assert not any(g.get_flows(k)[1].any() for k in every)
    _both(g, ref, [dict(n_users=0)], [0.104], cell_ids=[0], what="the same clock again")
    assert _counters(g) == before
    _both(g, ref, [plain_flows_call(90 + k, uid, fb) for k in every], 0.106, what="full call after the empty ones")
    assert _counters(g) != before
    assert g.launch_count == ref.launch_count == 5
    code, msg = g.flows_jit_status()
    assert code == 1 and f"lean build: 5 checked call(s) agreed with {REF}, 3 to go" in msg, (code, msg)
    g.close()
    ref.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. subsets, permutations and cqi_epoch modes mixed in one launch
# ---------------------------------------------------------------------------------------------------------------------------

def _image_plan(run, n_tti=40, seed=31):
    """The launches of the test below and what they do to the cells' CQI images, from the oracle's record alone (the rules of
    tests/test_gpu_group_flows.py): per TTI the parts, the totals (reused, stored, without a promise), launches with all three modes."""
    rng = np.random.default_rng(seed)
    image = [None] * CELLS
    want, mixed, plan = [0, 0, 0], 0, []
    for t, row in enumerate(run["steps"][:n_tti]):
        order = [int(x) for x in rng.permutation(CELLS)]
        parts = [order] if t % 3 == 0 else [order[:1], order[1:]]
        plan.append(parts)
        for part in parts:
            modes = set()
            for k in part:
                st = row[k]
                if len(st["uid"]) == 0:
                    continue
                epoch = 0 if k == 1 else st["epoch"]
                key = (epoch, BITS(st["uid"]))
                mode = 0 if epoch == 0 else (2 if image[k] == key else 1)
                want[{2: 0, 1: 1, 0: 2}[mode]] += 1
                image[k] = key if mode else None
                modes.add(mode)
            mixed += len(modes) == 3
    return plan, tuple(want), mixed


def test_subsets_permutations_and_image_modes(rs, oracle, monkeypatch):
    monkeypatch.setenv("RS_JIT_SELFCHECK", "2")
    run = _run(oracle)
    plan, want, mixed = _image_plan(run)
    assert all(w > 0 for w in want) and mixed > 0, (want, mixed)   # (of the inputs alone)
    ref, g = make_group(rs), make_group(rs)
    g.specialize_flows()
    set_all_flows(g, run)
    set_all_flows(ref, run)
    launches = 0
    for t, row in enumerate(run["steps"][:len(plan)]):
        for part in plan[t]:
            others = [k for k in range(CELLS) if k not in part]
            before = [flows_bits(g, k) for k in others]
            calls = [flows_call(row[k], epoch=0 if k == 1 else row[k]["epoch"]) for k in part]
            res = _both(g, ref, calls, run["ticks"][t], cell_ids=part, what=f"TTI {t} cells {part}", state=t % 8 == 0)
            launches += 1
            for r, k in zip(res, part):
                same_as_oracle(r, row[k], f"TTI {t} cell {k} (parts {plan[t]})")
            assert before == [flows_bits(g, k) for k in others], f"TTI {t}: a cell the call did not name moved"
        if t + 1 in run["state"]:
            _same_state(g, ref, range(CELLS), f"after TTI {t + 1}")
            for k in range(CELLS):
                a, _, last, cb, cr = g.get_flows(k)
                has = run["kinds"][k] != 0
                assert BITS(a[:USERS][has]) == BITS(run["state"][t + 1][k][has]) and last == run["ticks"][t]
                np.testing.assert_array_equal(cb[:USERS], run["cum_bytes"][t + 1][k])
                np.testing.assert_array_equal(cr[:USERS], run["cum_rbs"][t + 1][k])
    assert g.image_stats == ref.image_stats == want
    assert g.launch_count == ref.launch_count == launches and g.kernel_name == JIT_NAME
    g.close()
    ref.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. names and independence of scheduler 1's pairs; 7. a build that is wrong in a counter alone
# ---------------------------------------------------------------------------------------------------------------------------

UID, FB = [0, 0, 1, 2, 5, 7, 7], [0, 1, 1, 0, 1, 0, 1]


def _three_forms(rs, rng, g, ref, it, flows_jit=True, others_jit=True):
    """A plain call on every cell, a resident call on cell 2, a flows call on cells 1 and 0: each on its own entry point."""
    plain = [dict(cqi=synth_cqi(500 + 10 * it + k, (CAP, R_SMALL), HIST), avg_rate=rng.uniform(1e3, 5e6, CAP), data_to_transmit=np.full(CAP, 3000, np.int32))
             for k in range(CELLS)]
    for a, b in zip(g.schedule_tti(plain), ref.schedule_tti(plain)):
        _same_results(a, b, f"round {it}: plain call")
    assert g.kernel_name == ("rs_group_kernel_jit" if others_jit else "rs_group_kernel<1, 0>")
    at = [dict(cqi=synth_cqi(600 + it, (CAP, R_SMALL), HIST))]
    now = 0.101 + 0.001 * it
    _same_results(g.schedule_tti_at(at, now, cell_ids=[2])[0], ref.schedule_tti_at(at, now, cell_ids=[2])[0], f"round {it}: resident call")
    assert g.kernel_name == ("rs_group_resident_kernel_jit" if others_jit else "rs_group_resident_kernel<1, 0>")
    assert all(BITS(x) == BITS(y) for x, y in zip(g.get_avg(2)[:2], ref.get_avg(2)[:2])), f"round {it}: resident stores"
    return _both(g, ref, [plain_flows_call(700 + 10 * it + k, UID, FB, data=300 + 40 * k) for k in range(2)], now, cell_ids=[1, 0],
                 what=f"round {it}: flows call", jit=flows_jit)


def _three_pairs(rs, rng, others=True):
    """scheduler 1 has three of the five forms (the queued and the counted form are the transport schedulers' and scheduler 7's)"""
    ref = make_group(rs)
    g = rs.GroupScheduler(rs.SliceConfig([CAP]), R_SMALL, G_SMALL, CELLS, sched=SCHED_PF, jit=others, jit_resident=others, jit_flows=True)
    has = np.ones((CAP, 2), bool)
    a0 = rng.uniform(1e3, 5e6, CAP)
    for grp in (g, ref):
        for k in range(2):
            grp.set_flows(k, has, np.stack([a0, a0[::-1]], axis=1), 0.1)
        grp.set_avg(2, a0, 0.1)
    return g, ref


def _statuses(g):
    return (g.jit_status()[0], g.resident_jit_status()[0], g.queued_jit_status()[0], g.counted_jit_status()[0], g.flows_jit_status()[0])


def test_names_and_independence_of_the_pairs(rs, monkeypatch):
    monkeypatch.setenv("RS_JIT_SELFCHECK", "2")
    rng = np.random.default_rng(61)
    g, ref = _three_pairs(rs, rng)
    assert _statuses(g) == (1, 1, 0, 0, 1)
    for it in range(3):
        _three_forms(rs, rng, g, ref, it)
    assert "3 checked call(s) agreed with the built-in kernel field by field, 5 to go" in g.jit_status()[1], g.jit_status()
    assert "lean build: 3 checked call(s) agreed with the built-in resident kernel" in g.resident_jit_status()[1], g.resident_jit_status()
    assert f"lean build: 3 checked call(s) agreed with {REF}, 5 to go" in g.flows_jit_status()[1], g.flows_jit_status()
    assert g.launch_count == 9
    stats = rs.jit_cache_stats()
    g.specialize_flows()   # RS_OK, nothing built
    assert rs.jit_cache_stats() == stats
    g.close()
    ref.close()
    # specialize_flows() later, between two calls: no state is touched; the queued and the counted pair do not exist for scheduler 1,
    # the flows pair for no other scheduler
    g, ref = make_group(rs), make_group(rs)
    for grp in (g, ref):
        grp.set_flows(0, np.ones((CAP, 2), bool), np.full((CAP, 2), 2e5), 0.1)
    _both(g, ref, [plain_flows_call(800, UID, FB)], 0.101, cell_ids=[0], what="before specialize_flows", jit=False)
    before = flows_bits(g, 0) + BITS(g.slice_offset(0))
    g.specialize_flows()
    assert flows_bits(g, 0) + BITS(g.slice_offset(0)) == before
    _both(g, ref, [plain_flows_call(801, UID, FB)], 0.102, cell_ids=[0], what="after specialize_flows")
    for name in ("specialize_queued", "specialize_counted"):
        with pytest.raises(rs.RadioSaberError) as e:
            getattr(g, name)()
        assert e.value.code == -1
    assert _statuses(g) == (0, 0, 0, 0, 1)
    g.close()
    ref.close()
    for sched in (9, 7):
        g = make_group(rs, sched=sched)
        with pytest.raises(rs.RadioSaberError) as e:
            g.specialize_flows()
        assert e.value.code == -1 and g.flows_jit_status()[0] == 0   # RS_ERR_INVALID
        g.close()


def test_a_wrong_flows_build_is_dropped_on_the_counters_alone(rs, monkeypatch, tmp_path):
    """-DRS_FAULT_INJECT_FLOWS: the run-time flows kernel adds a byte more to cum_bytes of every flow it credits (a wrong value, no
    address).  Outputs, averages and pending bytes are right; the first call's comparison of the counters drops the flows pair, and
    it alone."""
    monkeypatch.delenv("RS_JIT_SELFCHECK", raising=False)
    monkeypatch.setenv("RS_JIT_EXTRA", "-DRS_FAULT_INJECT_FLOWS")
    monkeypatch.setenv("RS_JIT_CACHE_DIR", str(tmp_path))
    rng = np.random.default_rng(66)
    g, ref = _three_pairs(rs, rng)
    assert _statuses(g) == (1, 1, 0, 0, 1)
    files = set(tmp_path.glob("*.rsco"))
    assert len(files) == 6
    flows_files = {f for f in files if b"-DRS_JIT_GROUP_FLOWS=1" in f.read_bytes()}
    assert len(flows_files) == 2
    res = _three_forms(rs, rng, g, ref, 0, flows_jit=False)   # RS_OK; outputs and state: the built-in kernel's
    assert any(r.user_tbs_bits.any() for r in res)
    code, msg = g.flows_jit_status()
    assert code == -2 and "cum_bytes[" in msg and "cell " in msg and "checked call 1" in msg and "the built-in kernel's" in msg, (code, msg)
    assert "the built-in flows kernel serves" in msg, msg
    assert set(tmp_path.glob("*.rsco")) == files - flows_files, "the rejected flows builds are still in the cache"
    assert _statuses(g) == (1, 1, 0, 0, -2)   # the other pairs stay
    with pytest.raises(rs.RadioSaberError) as e:
        g.specialize_flows()
    assert e.value.code == -4 and "cum_bytes[" in str(e.value)   # RS_ERR_STATE, with the reason
    for it in range(1, 3):
        _three_forms(rs, rng, g, ref, it, flows_jit=False)
        assert g.kernel_name == BUILT_IN
    assert g.launch_count == ref.launch_count == 9
    g.close()
    ref.close()
    # the same wrong build without the check really leaves wrong byte counters (the injection bites)
    monkeypatch.setenv("RS_JIT_SELFCHECK", "0")
    monkeypatch.setenv("RS_JIT_EXTRA", "-DRS_FAULT_INJECT_FLOWS -DRS_UNCHECKED_TWIN")  # (another key: the first one is rejected for this process)
    g, ref = make_group(rs), make_group(rs)
    g.specialize_flows()
    for grp in (g, ref):
        grp.set_flows(0, np.ones((CAP, 2), bool), np.full((CAP, 2), 2e5), 0.1)
    res = _both(g, ref, [plain_flows_call(900, UID, FB)], 0.101, cell_ids=[0], what="unchecked wrong build", state=False)[0]   # the outputs are right ...
    mine, theirs = g.get_flows(0), ref.get_flows(0)
    assert BITS(mine[0]) == BITS(theirs[0]) and BITS(mine[1]) == BITS(theirs[1]) and BITS(mine[4]) == BITS(theirs[4])   # ... averages, pending bytes, cum_rbs too
    credited = np.zeros((CAP, 2), np.int64)
    credited[UID, FB] = res.user_tbs_bits // 8 > 0
    assert credited.any()
    np.testing.assert_array_equal(mine[3] - theirs[3], credited)   # ... the byte counters are not: one more per credited flow
    g.close()
    ref.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 8. the mark travels
# ---------------------------------------------------------------------------------------------------------------------------

CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(root)r + "/tests")
import numpy as np
import radiosaber_amd as rs
from conftest import synth_cqi
from test_group_queued_abi import CELLS, G_SMALL, HIST, R_SMALL, UES
FIELDS = ("target_rbs", "quota_rbgs", "rbg_to_user", "user_nprb", "user_final_cqi", "user_mcs", "user_tbs_bits")
CAP = 2 * sum(UES)
sc = rs.SliceConfig([CAP])
g = rs.GroupScheduler(sc, R_SMALL, G_SMALL, CELLS, sched=1)
g.specialize_flows()
ref = rs.GroupScheduler(sc, R_SMALL, G_SMALL, CELLS, sched=1)
rng = np.random.default_rng(6)
has = np.ones((CAP, 2), bool)
for k in range(CELLS):
    a0 = rng.uniform(1e3, 5e6, (CAP, 2))
    g.set_flows(k, has, a0, 0.1)
    ref.set_flows(k, has, a0, 0.1)
uid = np.repeat(np.arange(10, dtype=np.int32), 2)
fb = np.tile(np.array([0, 1], np.uint8), 10)
ok, names = True, set()
for it in range(16):   # 8 calls with per-RBG reports (the lean build), 8 with per-PRB reports (the general build)
    calls = []
    for k in range(CELLS):
        cqi = synth_cqi(600 + 10 * it + k, (len(uid), R_SMALL), HIST)
        kw = dict(cqi=cqi, user_id=uid, flow_bearer=fb, data_to_transmit=rng.choice(np.array([40, 300, 5000], np.int32), len(uid)))
        if it >= 8:
            kw = dict(kw, cqi=None, cqi_prb=np.repeat(cqi, G_SMALL, axis=1))
        calls.append(kw)
    if it %% 4 == 3:
        calls[1] = dict(n_users=0)
    res, want = g.schedule_tti_flows(calls, 0.101 + 0.001 * it), ref.schedule_tti_flows(calls, 0.101 + 0.001 * it)
    names.add(g.kernel_name)
    for k in range(CELLS):
        ok &= all(np.array_equal(getattr(res[k], f), getattr(want[k], f)) for f in FIELDS)
        ok &= all(np.array_equal(a, b) for a, b in zip(g.get_flows(k), ref.get_flows(k)))
        ok &= g.slice_offset(k).tobytes() == ref.slice_offset(k).tobytes()
out = dict(ok=bool(ok), status=g.flows_jit_status(), others=[g.jit_status()[0], g.resident_jit_status()[0], g.queued_jit_status()[0], g.counted_jit_status()[0]],
           kernels=sorted(names), launches=g.launch_count, stats=rs.jit_cache_stats(), counted=bool(g.get_flows(0)[3].any()))
g.close()
ref.close()
print(json.dumps(out))
"""


def _child(cache_dir):
    env = dict(os.environ, RS_JIT_CACHE_DIR=str(cache_dir), AMD_COMGR_CACHE="0")
    for k in ("RS_JIT_CACHE", "RS_JIT_SELFCHECK", "RS_JIT_EXTRA", "RS_JIT_LEAN", "RS_DROPIN_SELFCHECK_CALLS", "RS_DROPIN_COPY"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": str(ROOT)}], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().split("\n")[-1])


def test_the_self_check_mark_travels_to_the_next_process(rs, tmp_path):
    first = _child(tmp_path)
    assert first["ok"] and first["counted"] and first["status"][0] == 1 and first["kernels"] == [JIT_NAME] and first["launches"] == 16, first
    assert first["others"] == [0, 0, 0, 0], first
    assert f"general build: {VERIFIED}" in first["status"][1] and f"lean build: {VERIFIED}" in first["status"][1], first
    marks = sorted(f.read_bytes()[-8:].decode() for f in tmp_path.glob("*.rsco"))
    assert first["stats"]["misses"] == 2 and marks == ["VERIFIED", "VERIFIED"], (first, marks)
    second = _child(tmp_path)
    assert second["ok"] and second["stats"] == {"hits": 2, "misses": 0, "stores": 0, "rejected": 0}, second
    assert second["status"][0] == 1 and second["kernels"] == [JIT_NAME] and second["launches"] == 16, second
    assert "general build: carries the self-check mark" in second["status"][1] and "lean build: carries the self-check mark" in second["status"][1], second
    assert "agreed" not in second["status"][1], second   # no call was a checked one
