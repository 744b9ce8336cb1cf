"""rs_group_specialize_counted: a group's own run-time builds of the COUNTED kernel (entry point rs_group_counted_kernel_jit, general
and lean), checked against the built-in counted kernel on outputs, on the slots' sent rows AND on state -- slice state, both bearers'
averages, pending bytes, m_cumulateBytes and m_cumulateRBs of every user id, the last-update time.  Against an unspecialised twin and
against the oracle's DoSchedule() with queues on the scenario of tests/test_group_counted_abi.py, on the general build's paths, with
more positions than threads, with update-only launches, with subsets, permutations and cqi_epoch modes mixed in one launch, beside the
other four pairs, with builds that are wrong in a counter or in a sent row alone, and with the self-check mark that travels to the
next process.  Every comparison is bitwise."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import synth_cqi
from test_group_counted_abi import STATE_AT, counted_run
from test_group_queued_abi import CELLS, FIELDS, G_SMALL, HIST, INFINITE, R_SMALL, UES
from test_gpu_group_counted import BITS, counters_as_the_oracle, device_calls, make_group, same_as_oracle, simple_call, start

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
U_ALL = sum(UES)
FIRST = np.concatenate([[0], np.cumsum(UES)])
JIT_NAME = "rs_group_counted_kernel_jit"
REF = "the built-in counted kernel field by field, bearer stores, counters and sent rows included"
VERIFIED = f"verified (8 checked calls agreed with {REF})"
_RUNS = {}


@pytest.fixture(scope="module", autouse=True)
def cache_dir(tmp_path_factory):
    """The builds of this file go to a cache directory of its own: one hiprtc run per (shape, scheduler, build)."""
    mp = pytest.MonkeyPatch()
    d = tmp_path_factory.mktemp("counted_builds")
    mp.setenv("RS_JIT_CACHE_DIR", str(d))
    for k in ("RS_JIT_CACHE", "RS_JIT_EXTRA", "RS_JIT_LEAN", "RS_DROPIN_SELFCHECK_CALLS", "RS_JIT_SELFCHECK", "RS_DROPIN_COPY"):
        mp.delenv(k, raising=False)
    yield d
    mp.undo()


def _run(oracle, sched, **kw):
    key = (sched, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _RUNS:
        _RUNS[key] = counted_run(oracle, sched, **kw)
    return _RUNS[key]


def _same_results(res, want, what):
    for f in FIELDS:
        assert BITS(getattr(res, f)) == BITS(getattr(want, f)), f"{what}: {f}"
    assert res.sent.shape == want.sent.shape and BITS(res.sent) == BITS(want.sent), f"{what}: sent"


def _same_state(g, ref, cells, what):
    for k in cells:
        (a, p, l), (ra, rp, rl) = g.get_bearers(k), ref.get_bearers(k)
        assert BITS(a) == BITS(ra), f"{what}, cell {k}: avg"
        assert BITS(p) == BITS(rp), f"{what}, cell {k}: pending_bytes"
        assert l == rl, f"{what}, cell {k}: last_update"
        (cb, cr), (rcb, rcr) = g.get_counters(k), ref.get_counters(k)
        assert BITS(cb) == BITS(rcb), f"{what}, cell {k}: cum_bytes"
        assert BITS(cr) == BITS(rcr), f"{what}, cell {k}: cum_rbs"


def _same_slices(g, ref, cells, what):
    for k in cells:
        assert BITS(g.slice_offset(k)) == BITS(ref.slice_offset(k)), f"{what}, cell {k}: slice offsets"


def _both(g, ref, calls, now, cell_ids=None, what="", jit=True, state=True):
    """One counted call on the specialised group and on its unspecialised twin: outputs, sent rows, slice state, served-by name, and
    (state) the bearers and the counters."""
    res, want = g.schedule_tti_counted(calls, now, cell_ids=cell_ids), ref.schedule_tti_counted(calls, now, cell_ids=cell_ids)
    for j in range(len(calls)):
        _same_results(res[j], want[j], f"{what} slot {j}")
    assert g.kernel_name == (JIT_NAME if jit else ref.kernel_name), (g.kernel_name, g.counted_jit_status())
    cells = range(g.n_cells) if cell_ids is None else cell_ids
    _same_slices(g, ref, cells, what)
    if state:
        _same_state(g, ref, cells, what)
    return res


def _drive(g, ref, run, sched, what, permute=False, state_every=False, oracle_too=True):
    """counted_run's steps through both groups, the specialised one held against the oracle's record as well; permute: odd TTIs name
    the cells in reverse order."""
    K = len(run["kinds"])
    start(g, run)
    start(ref, run)
    for t, row in enumerate(run["steps"]):
        calls, ids = device_calls(sched, row), None
        if permute and t % 2:
            ids = list(range(K))[::-1]
            calls = [calls[k] for k in ids]
        at_state = (t + 1) in run["state"]
        res = _both(g, ref, calls, run["ticks"][t], cell_ids=ids, what=f"{what} TTI {t}", state=state_every or at_state)
        if oracle_too:
            for j, r in enumerate(res):
                k = j if ids is None else ids[j]
                same_as_oracle(r, row[k], f"{what} TTI {t} cell {k}")
            if at_state:
                counters_as_the_oracle(g, run, t + 1, what)
    assert g.launch_count == ref.launch_count == len(run["steps"])  # the twin launch of a checked call is not counted


# ---------------------------------------------------------------------------------------------------------------------------
# 1. equal to the built-in counted kernel and to the oracle
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("selfcheck", ["2", "0"])
@pytest.mark.parametrize("sched", [8, 9, 7, 103])
def test_equal_to_the_built_in_counted_kernel_and_to_the_oracle(rs, oracle, sched, selfcheck, monkeypatch):
    monkeypatch.setenv("RS_JIT_SELFCHECK", selfcheck)
    run = _run(oracle, sched)
    ref = make_group(rs, sched)
    g = make_group(rs, sched)
    g.specialize_counted()
    assert g.counted_jit_status()[0] == 1, g.counted_jit_status()
    assert (g.jit_status()[0], g.resident_jit_status()[0], g.queued_jit_status()[0], g.flows_jit_status()[0]) == (0, 0, 0, 0)
    _drive(g, ref, run, sched, f"sched {sched}")
    assert set(run["state"]) == set(STATE_AT)
    code, msg = g.counted_jit_status()
    assert code == 1, (code, msg)
    # (scheduler 7's calls carry required_rbs, the gate: the general build serves them; the others' calls are plain)
    served = "general" if sched == 7 else "lean"
    if selfcheck == "2":
        assert f"{served} build: {VERIFIED}" in msg, msg
    else:
        assert "agreed" not in msg, msg
    g.close()
    ref.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the general build's paths
# ---------------------------------------------------------------------------------------------------------------------------

def _random_calls(rng, has, t, sched, variant, seed):
    """One call's dictionaries: random data words on the existing bearers, the users with data (scheduler 7: of one slice per cell)."""
    calls = []
    for k in range(CELLS):
        data = np.where(has[k], rng.choice(np.array([0, 0, 37, 300, 2000, INFINITE], np.int32), (U_ALL, 2)), 0).astype(np.int32)
        if sched == 7:
            s = (t + k) % len(UES)
            data[:FIRST[s]] = 0
            data[FIRST[s + 1]:] = 0
            lo = int(FIRST[s])
        else:
            lo = 0
        if not data.any():
            data[lo, 0] = 500   # (bearer 0 exists for every user of these tests)
        ids = np.nonzero(data.any(axis=1))[0].astype(np.int32)
        n = len(ids)
        cqi = synth_cqi(seed + 10 * t + k, (n, R_SMALL), HIST)
        kw = dict(cqi=cqi, user_id=ids, rand0=int(rng.integers(0, 2**31 - 1)), rand1=int(rng.integers(0, 2**31 - 1)), data_to_transmit=data[ids])
        if variant == "custom":
            kw.update(hol_delay=rng.uniform(1e-5, 0.4, n), prio_has_data=(rng.random(n) < 0.8).astype(np.uint8))
        if variant == "prb":
            prb = np.repeat(cqi, G_SMALL, axis=1)
            prb[:, 1::G_SMALL] = np.maximum(1, prb[:, 1::G_SMALL] - 1)
            kw.update(cqi=None, cqi_prb=prb, cqi_epoch=1 + t // 2)   # stored, then served from the cell's per-PRB store
        if variant == "gates":
            kw.update(required_rbs=rng.integers(1, 3 * G_SMALL, n).astype(np.int32))
        calls.append(kw)
    return calls


def _bearers(rng):
    has = [rng.random((U_ALL, 2)) < 0.75 for _ in range(CELLS)]
    for h in has:
        h[:, 0] = True
    return has, [np.where(h, rng.uniform(1e3, 5e6, (U_ALL, 2)), 0.0) for h in has]


@pytest.mark.parametrize("sched,variant", [(9, "custom"), (9, "prb"), (7, "gates")])
def test_general_build_paths(rs, sched, variant, monkeypatch):
    """Customised slices (algo_alpha = 1, hol_delay, prio_has_data), per-PRB reports on the staged-copy path, scheduler 7's required_rbs:
    5 such calls, then 3 plain ones.  The lean build serves none of the former and all of the latter -- but a config with customised
    slices has no plain call."""
    monkeypatch.setenv("RS_JIT_SELFCHECK", "2")
    if variant == "prb":
        monkeypatch.setenv("RS_DROPIN_COPY", "1")
    cfg = dict(algo_alpha=[1, 1, 1], algo_beta=[1, 1, 1]) if variant == "custom" else {}
    ref, g = make_group(rs, sched, **cfg), make_group(rs, sched, **cfg)
    g.specialize_counted()
    rng = np.random.default_rng(400 + sched + len(variant))
    has, avg = _bearers(rng)
    for k in range(CELLS):
        for grp in (g, ref):
            grp.set_bearers(k, has[k], avg[k], 0.1)
            grp.set_counters(k)
    for t in range(5):
        _both(g, ref, _random_calls(rng, has, t, sched, variant, 3000), 0.101 + 0.001 * t, what=f"{variant} call {t}")
    code, msg = g.counted_jit_status()
    assert code == 1 and f"general build: 5 checked call(s) agreed with {REF}, 3 to go" in msg and "lean build: 0 checked call(s) agreed" in msg, msg
    for t in range(5, 8):
        _both(g, ref, _random_calls(rng, has, t, sched, "custom" if variant == "custom" else None, 3000), 0.101 + 0.001 * t, what=f"plain call {t}")
    code, msg = g.counted_jit_status()
    if variant == "custom":
        assert code == 1 and f"general build: {VERIFIED}" in msg and "lean build: 0 checked call(s) agreed" in msg, msg
    else:
        assert code == 1 and "general build: 5 checked call(s) agreed" in msg and "lean build: 3 checked call(s) agreed" in msg, msg
    assert any(x.any() for k in range(CELLS) for x in g.get_counters(k))
    assert g.launch_count == ref.launch_count == 8
    g.close()
    ref.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. more positions than threads, user_id subsets, permuted cell_ids
# ---------------------------------------------------------------------------------------------------------------------------

def test_more_positions_than_threads_and_permuted_cells(rs, oracle, monkeypatch):
    """2 x 350 users (the shape of tests/test_gpu_group_counted.py): the constant-stride update covers 1 400 bearers, gather and credit
    up to 700 call positions; every call names a user_id subset (the active users), odd TTIs name the cells in reverse order.  A
    position past the 512th is credited: the second pass of the constant-stride loop wrote its counters and its sent row."""
    monkeypatch.setenv("RS_JIT_SELFCHECK", "2")
    kw = dict(ues=[350, 350], R=4, G=2, K=2)
    run = _run(oracle, 9, n_tti=12, grid_every=5, seed=3, busy=0.5, state_at=(1, 2, 12), **kw)
    sizes = [len(st["ids"]) for row in run["steps"] for st in row]
    assert max(sizes) > 512 and min(sizes) < 700
    ref, g = make_group(rs, 9, **kw), make_group(rs, 9, **kw)
    g.specialize_counted()
    K = 2
    start(g, run)
    start(ref, run)
    beyond = 0
    for t, row in enumerate(run["steps"]):
        calls, ids = device_calls(9, row), list(range(K))
        if t % 2:
            ids = ids[::-1]
            calls = [calls[k] for k in ids]
        res = _both(g, ref, calls, run["ticks"][t], cell_ids=ids, what=f"700 users TTI {t}")
        for j, r in enumerate(res):
            same_as_oracle(r, row[ids[j]], f"700 users TTI {t} cell {ids[j]}")
            beyond += int((r.sent[512:] > 0).any(axis=1).sum())
        if t + 1 in run["state"]:
            counters_as_the_oracle(g, run, t + 1, "700 users")
    assert beyond > 0, "no position past the 512th was credited"
    assert g.kernel_name == JIT_NAME and g.launch_count == ref.launch_count == 12
    code, msg = g.counted_jit_status()
    assert code == 1 and f"lean build: {VERIFIED}" in msg, (code, msg)
    g.close()
    ref.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. update-only launches
# ---------------------------------------------------------------------------------------------------------------------------

def _counters(g, cells=range(CELLS)):
    return b"".join(BITS(x) for k in cells for x in g.get_counters(k))


def test_update_only_launches(rs, monkeypatch):
    monkeypatch.setenv("RS_JIT_SELFCHECK", "2")
    ref, g = make_group(rs, 9), make_group(rs, 9)
    g.specialize_counted()
    rng = np.random.default_rng(7)
    has = np.ones((U_ALL, 2), bool)
    has[3] = (True, False)
    for k in range(CELLS):
        for grp in (g, ref):
            grp.set_bearers(k, has, np.full((U_ALL, 2), 2e5), 0.1)
            grp.set_counters(k)
    every = range(CELLS)
    res = _both(g, ref, [simple_call(rng, 70 + k, U_ALL) for k in every], 0.101, what="full call")
    assert all(r.sent.any() for r in res) and all(g.get_bearers(k)[1].any() for k in every)
    # a mixed call inside the checked ones: cell 1 has nobody to schedule -- none of its counters moves, no sent row is written
    before = _counters(g, [1])
    res = _both(g, ref, [simple_call(rng, 80, U_ALL), dict(n_users=0), simple_call(rng, 82, U_ALL)], 0.102, what="mixed call")
    assert (res[1].rbg_to_user == -1).all() and not res[1].target_rbs.any() and (res[0].rbg_to_user >= 0).any()
    assert res[1].sent.shape == (0, 2) and _counters(g, [1]) == before
    assert not g.get_bearers(1)[1].any() and g.get_bearers(1)[2] == 0.102
    # empty slots only, named out of order, a clock per cell: one launch, a checked call like any other, no counter moves
    before = _counters(g)
    res = _both(g, ref, [dict(n_users=0)] * CELLS, [0.103, 0.104, 0.105], cell_ids=[2, 0, 1], what="empty slots only")
    assert all(r.sent.shape == (0, 2) for r in res) and _counters(g) == before
    assert [g.get_bearers(k)[2] for k in every] == [0.104, 0.105, 0.103]
    assert not any(g.get_bearers(k)[1].any() for k in every)
    _both(g, ref, [dict(n_users=0)], [0.104], cell_ids=[0], what="the same clock again")
    assert _counters(g) == before
    _both(g, ref, [simple_call(rng, 90 + k, U_ALL) for k in every], 0.106, what="full call after the empty ones")
    assert _counters(g) != before
    assert g.launch_count == ref.launch_count == 5
    code, msg = g.counted_jit_status()
    assert code == 1 and f"lean build: 5 checked call(s) agreed with {REF}, 3 to go" in msg, (code, msg)
    g.close()
    ref.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. subsets, permutations and cqi_epoch modes mixed in one launch
# ---------------------------------------------------------------------------------------------------------------------------

def _image_plan(run, n_tti=40, seed=31):
    """The launches of the test below and what they do to the cells' CQI images, from the oracle's record alone: per TTI the parts
    (lists of cells), and the totals (reused, stored, without a promise) and the number of launches that mix all three modes."""
    rng = np.random.default_rng(seed)
    image = [None] * CELLS  # the mirror of the cells' image records: (epoch, user list) of the last stored call
    want, mixed, plan = [0, 0, 0], 0, []
    for t, row in enumerate(run["steps"][:n_tti]):
        order = [int(x) for x in rng.permutation(CELLS)]
        parts = [order] if t % 3 == 0 else [order[:1], order[1:]]
        plan.append(parts)
        for part in parts:
            modes = set()
            for k in part:
                st = row[k]
                if len(st["ids"]) == 0:
                    continue
                key = (st["epoch"], BITS(st["ids"]))
                mode = 0 if k == 1 else (2 if image[k] == key else 1)
                want[{2: 0, 1: 1, 0: 2}[mode]] += 1
                image[k] = key if mode else None
                modes.add(mode)
            mixed += len(modes) == 3
    return plan, tuple(want), mixed


def test_subsets_permutations_and_image_modes(rs, oracle, monkeypatch):
    """The oracle's record served in changing order and in subsets through the specialised builds.  Cell 1 promises nothing (cqi_epoch
    0, mode 0), cells 0 and 2 number their reports: mode 1 when number or user list changed, mode 2 otherwise."""
    monkeypatch.setenv("RS_JIT_SELFCHECK", "2")
    run = _run(oracle, 9)
    plan, want, mixed = _image_plan(run)
    assert all(w > 0 for w in want) and mixed > 0, (want, mixed)   # (of the inputs alone: every mode occurs, and all three in one launch)
    ref, g = make_group(rs, 9), make_group(rs, 9)
    g.specialize_counted()
    start(g, run)
    start(ref, run)
    launches = 0
    for t, row in enumerate(run["steps"][:len(plan)]):
        calls_all = device_calls(9, row)
        calls_all[1].pop("cqi_epoch", None)
        for part in plan[t]:
            res = _both(g, ref, [calls_all[k] for k in part], run["ticks"][t], cell_ids=part, what=f"TTI {t} cells {part}", state=t % 8 == 0)
            launches += 1
            for r, k in zip(res, part):
                same_as_oracle(r, row[k], f"TTI {t} cell {k} (parts {plan[t]})")
        if t + 1 in run["state"]:
            counters_as_the_oracle(g, run, t + 1, "subsets")
    assert g.image_stats == ref.image_stats == want
    assert g.launch_count == ref.launch_count == launches and g.kernel_name == JIT_NAME
    g.close()
    ref.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. names and independence of the pairs; 7. builds that are wrong in a counter or in a sent row alone
# ---------------------------------------------------------------------------------------------------------------------------

def _four_forms(rs, rng, g, ref, it, counted_jit=True, queued_jit=True, others_jit=True):
    """A plain call on every cell, a resident call on cell 2, a queued call on cell 1 and a counted call on cells 1 and 0: each on its
    own entry point."""
    plain = [dict(cqi=synth_cqi(500 + 10 * it + k, (U_ALL, R_SMALL), HIST), avg_rate=rng.uniform(1e3, 5e6, U_ALL), rand0=3 + it, rand1=4 + k)
             for k in range(CELLS)]
    for a, b in zip(g.schedule_tti(plain), ref.schedule_tti(plain)):
        for f in FIELDS:
            assert BITS(getattr(a, f)) == BITS(getattr(b, f)), f"round {it}: plain call: {f}"
    assert g.kernel_name == ("rs_group_kernel_jit" if others_jit else ref.kernel_name)
    at = [dict(cqi=synth_cqi(600 + it, (U_ALL, R_SMALL), HIST), rand0=5 + it, rand1=6)]
    now = 0.101 + 0.002 * it
    a, b = g.schedule_tti_at(at, now, cell_ids=[2])[0], ref.schedule_tti_at(at, now, cell_ids=[2])[0]
    assert all(BITS(getattr(a, f)) == BITS(getattr(b, f)) for f in FIELDS), f"round {it}: resident call"
    assert g.kernel_name == ("rs_group_resident_kernel_jit" if others_jit else ref.kernel_name)
    data = np.tile(np.array([300, 900], np.int32), (U_ALL, 1))
    q = [simple_call(rng, 650 + it, U_ALL, data)]
    a, b = g.schedule_tti_queued(q, now, cell_ids=[1])[0], ref.schedule_tti_queued(q, now, cell_ids=[1])[0]
    assert all(BITS(getattr(a, f)) == BITS(getattr(b, f)) for f in FIELDS) and a.sent is None, f"round {it}: queued call"
    assert g.kernel_name == ("rs_group_queued_kernel_jit" if queued_jit else ref.kernel_name)
    return _both(g, ref, [simple_call(rng, 700 + 10 * it + k, U_ALL, data) for k in range(2)], now + 0.001, cell_ids=[1, 0], what=f"round {it}: counted call",
                 jit=counted_jit)


def _four_pairs(rs, rng, others=True):
    """others = False: the queued and the counted pair alone (four builds instead of eight)"""
    ref = make_group(rs, 9)
    g = rs.GroupScheduler(rs.SliceConfig(UES), R_SMALL, G_SMALL, CELLS, sched=9, jit=others, jit_resident=others, jit_queued=True, jit_counted=True)
    a0 = rng.uniform(1e3, 5e6, U_ALL)
    for grp in (g, ref):
        for k in range(2):
            grp.set_bearers(k, np.ones((U_ALL, 2), bool), np.stack([a0, a0[::-1]], axis=1), 0.1)
            grp.set_counters(k)
        grp.set_avg(2, a0, 0.1)
    return g, ref


def _statuses(g):
    return (g.jit_status()[0], g.resident_jit_status()[0], g.queued_jit_status()[0], g.counted_jit_status()[0], g.flows_jit_status()[0])


def test_names_and_independence_of_the_pairs(rs, monkeypatch):
    """Scheduler 9 has four of the five forms (the flows form is scheduler 1's: tests/test_gpu_group_flows_specialize.py builds all of
    scheduler 1's pairs): every call names its own kernel, every status reports its own pair only."""
    monkeypatch.setenv("RS_JIT_SELFCHECK", "2")
    rng = np.random.default_rng(61)
    g, ref = _four_pairs(rs, rng)
    assert _statuses(g) == (1, 1, 1, 1, 0)
    for it in range(3):
        _four_forms(rs, rng, g, ref, it)
    assert "lean build: 3 checked call(s) agreed with the built-in kernel field by field, 5 to go" in g.jit_status()[1], g.jit_status()
    assert "lean build: 3 checked call(s) agreed with the built-in resident kernel" in g.resident_jit_status()[1], g.resident_jit_status()
    assert "lean build: 3 checked call(s) agreed with the built-in queued kernel" in g.queued_jit_status()[1], g.queued_jit_status()
    assert f"lean build: 3 checked call(s) agreed with {REF}, 5 to go" in g.counted_jit_status()[1], g.counted_jit_status()
    assert g.launch_count == 12
    stats = rs.jit_cache_stats()
    g.specialize_counted()   # RS_OK, nothing built
    assert rs.jit_cache_stats() == stats
    g.close()
    ref.close()
    # specialize_counted() later, between two calls: no state is touched, and queued calls stay on the built-in queued kernel;
    # specialize_queued() does not reach counted calls (tests/test_gpu_group_counted.py); schedulers without the form are refused
    g, ref = make_group(rs, 9), make_group(rs, 9)
    for grp in (g, ref):
        grp.set_bearers(0, np.ones((U_ALL, 2), bool), np.full((U_ALL, 2), 2e5), 0.1)
        grp.set_counters(0)
    _both(g, ref, [simple_call(rng, 800, U_ALL)], 0.101, cell_ids=[0], what="before specialize_counted", jit=False)
    before = [BITS(x) for x in g.get_bearers(0)[:2]] + [BITS(g.slice_offset(0)), _counters(g, [0])]
    g.specialize_counted()
    assert [BITS(x) for x in g.get_bearers(0)[:2]] + [BITS(g.slice_offset(0)), _counters(g, [0])] == before
    _both(g, ref, [simple_call(rng, 801, U_ALL)], 0.102, cell_ids=[0], what="after specialize_counted")
    g.schedule_tti_queued([simple_call(rng, 802, U_ALL)], 0.103, cell_ids=[0])
    assert g.kernel_name.startswith("rs_group_queued_kernel<9,") and g.queued_jit_status()[0] == 0
    g.close()
    ref.close()
    for sched in (10, 1):
        g = make_group(rs, sched)
        with pytest.raises(rs.RadioSaberError) as e:
            g.specialize_counted()
        assert e.value.code == -1 and g.counted_jit_status()[0] == 0   # RS_ERR_INVALID
        g.close()


@pytest.mark.parametrize("switch,field", [("1", "cum_rbs["), ("2", "sent[")])
def test_a_wrong_counted_build_is_dropped_on_what_only_the_new_comparison_sees(rs, monkeypatch, tmp_path, switch, field):
    """-DRS_FAULT_INJECT_COUNTED=1: the run-time counted kernel adds one PRB more to cum_rbs of the last bearer it credits for a position;
    =2: that bearer's entry of the position's sent row is a byte more while pending bytes and counters stay right (wrong values, no
    address).  Outputs and bearer stores are right; the first call's comparison of the counters / of the sent rows drops the counted
    pair, and it alone."""
    monkeypatch.delenv("RS_JIT_SELFCHECK", raising=False)
    monkeypatch.setenv("RS_JIT_EXTRA", f"-DRS_FAULT_INJECT_COUNTED={switch}")
    monkeypatch.setenv("RS_JIT_CACHE_DIR", str(tmp_path))
    rng = np.random.default_rng(66)
    g, ref = _four_pairs(rs, rng, others=False)
    assert _statuses(g) == (0, 0, 1, 1, 0)
    files = set(tmp_path.glob("*.rsco"))
    assert len(files) == 4
    counted_files = {f for f in files if b"-DRS_JIT_GROUP_COUNTED=1" in f.read_bytes()}
    assert len(counted_files) == 2
    res = _four_forms(rs, rng, g, ref, 0, counted_jit=False, others_jit=False)   # RS_OK; outputs, sent rows and state: the built-in kernel's
    assert any(r.sent.any() for r in res)
    code, msg = g.counted_jit_status()
    assert code == -2 and field in msg and "cell " in msg and "checked call 1" in msg and "the built-in kernel's" in msg, (code, msg)
    assert "the built-in counted kernel serves" in msg, msg
    assert set(tmp_path.glob("*.rsco")) == files - counted_files, "the rejected counted builds are still in the cache"
    assert _statuses(g) == (0, 0, 1, -2, 0)   # the queued pair stays
    with pytest.raises(rs.RadioSaberError) as e:
        g.specialize_counted()
    assert e.value.code == -4 and field in str(e.value)   # RS_ERR_STATE, with the reason
    for it in range(1, 3):
        _four_forms(rs, rng, g, ref, it, counted_jit=False, others_jit=False)
        assert g.kernel_name.startswith("rs_group_counted_kernel<9,")
    assert g.launch_count == ref.launch_count == 12
    g.close()
    ref.close()
    # the same wrong build without the check really leaves the wrong value (the injection bites)
    monkeypatch.setenv("RS_JIT_SELFCHECK", "0")
    monkeypatch.setenv("RS_JIT_EXTRA", f"-DRS_FAULT_INJECT_COUNTED={switch} -DRS_UNCHECKED_TWIN")  # (another key: the first one is rejected for this process)
    g, ref = make_group(rs, 9), make_group(rs, 9)
    g.specialize_counted()
    for grp in (g, ref):
        grp.set_bearers(0, np.ones((U_ALL, 2), bool), np.full((U_ALL, 2), 2e5), 0.1)
        grp.set_counters(0)
    data = np.tile(np.array([300, 40], np.int32), (U_ALL, 1))
    call = [simple_call(rng, 900, U_ALL, data)]
    mine, theirs = g.schedule_tti_counted(call, 0.101, cell_ids=[0])[0], ref.schedule_tti_counted(call, 0.101, cell_ids=[0])[0]
    assert g.kernel_name == JIT_NAME
    for f in FIELDS:   # the outputs are right ...
        assert BITS(getattr(mine, f)) == BITS(getattr(theirs, f)), f
    assert all(BITS(x) == BITS(y) for x, y in zip(g.get_bearers(0), ref.get_bearers(0)))   # ... and so are the bearer stores
    (cb, cr), (rcb, rcr) = g.get_counters(0), ref.get_counters(0)
    served = theirs.sent.any(axis=1)
    last = np.where(theirs.sent[:, 0] > 0, 0, 1)   # the last bearer credited: bearer 0 when it got anything
    assert served.any() and BITS(cb) == BITS(rcb)
    extra = np.zeros((U_ALL, 2), np.int64)
    extra[np.arange(U_ALL), last] = served
    if switch == "1":
        np.testing.assert_array_equal(cr - rcr, extra)
        assert BITS(mine.sent) == BITS(theirs.sent)
    else:
        np.testing.assert_array_equal(mine.sent - theirs.sent, extra)
        assert BITS(cr) == BITS(rcr)
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
from test_group_queued_abi import CELLS, FIELDS, G_SMALL, HIST, R_SMALL, UES
U = sum(UES)
sc = rs.SliceConfig(UES)
g = rs.GroupScheduler(sc, R_SMALL, G_SMALL, CELLS, sched=9)
g.specialize_counted()
ref = rs.GroupScheduler(sc, R_SMALL, G_SMALL, CELLS, sched=9)
rng = np.random.default_rng(6)
has = np.ones((U, 2), bool)
for k in range(CELLS):
    a0 = rng.uniform(1e3, 5e6, (U, 2))
    for grp in (g, ref):
        grp.set_bearers(k, has, a0, 0.1)
        grp.set_counters(k)
ok, names = True, set()
for it in range(16):   # 8 plain calls (the lean build), 8 with per-PRB reports (the general build)
    calls = []
    for k in range(CELLS):
        cqi = synth_cqi(600 + 10 * it + k, (U, R_SMALL), HIST)
        kw = dict(cqi=cqi, rand0=int(rng.integers(0, 2**31 - 1)), rand1=int(rng.integers(0, 2**31 - 1)),
                  data_to_transmit=rng.choice(np.array([40, 300, 5000], np.int32), (U, 2)))
        if it >= 8:
            kw = dict(kw, cqi=None, cqi_prb=np.repeat(cqi, G_SMALL, axis=1))
        calls.append(kw)
    if it %% 4 == 3:
        calls[1] = dict(n_users=0)
    res, want = g.schedule_tti_counted(calls, 0.101 + 0.001 * it), ref.schedule_tti_counted(calls, 0.101 + 0.001 * it)
    names.add(g.kernel_name)
    for k in range(CELLS):
        ok &= all(np.array_equal(getattr(res[k], f), getattr(want[k], f)) for f in FIELDS) and np.array_equal(res[k].sent, want[k].sent)
        ok &= all(np.array_equal(a, b) for a, b in zip(g.get_bearers(k), ref.get_bearers(k)))
        ok &= all(np.array_equal(a, b) for a, b in zip(g.get_counters(k), ref.get_counters(k)))
        ok &= g.slice_offset(k).tobytes() == ref.slice_offset(k).tobytes()
out = dict(ok=bool(ok), status=g.counted_jit_status(), others=[g.jit_status()[0], g.resident_jit_status()[0], g.queued_jit_status()[0], g.flows_jit_status()[0]],
           kernels=sorted(names), launches=g.launch_count, stats=rs.jit_cache_stats(), counted=bool(g.get_counters(0)[0].any()))
g.close()
ref.close()
print(json.dumps(out))
"""


def _child(cache_dir):
    env = dict(os.environ, RS_JIT_CACHE_DIR=str(cache_dir), AMD_COMGR_CACHE="0")
    for k in ("RS_JIT_CACHE", "RS_JIT_SELFCHECK", "RS_JIT_EXTRA", "RS_JIT_LEAN", "RS_DROPIN_SELFCHECK_CALLS"):
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
