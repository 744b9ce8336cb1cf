"""rs_group_specialize_queued: a group's own run-time builds of the QUEUED kernel (entry point rs_group_queued_kernel_jit, general and
lean), checked against the built-in queued kernel on outputs AND on state -- slice state, both bearers' averages and pending bytes of
every user id, the last-update time.  Against an unspecialised twin and against the oracle's DoSchedule() with queues on the scenario
of tests/test_group_queued_abi.py, on the general build's paths, with more bearers than threads, with update-only launches, beside
the other two pairs, with a build that is wrong in its bearer stores alone, and with the self-check mark that travels to the next
process.  Every comparison is bitwise."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import synth_cqi
from test_group_queued_abi import CELLS, FIELDS, G_SMALL, HIST, INFINITE, R_SMALL, STATE_AT, UES, binding_counts, oracle_run
from test_gpu_group_queued import BITS, device_calls, follow_the_oracle, make_group, simple_call

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
U_ALL = sum(UES)
FIRST = np.concatenate([[0], np.cumsum(UES)])
JIT_NAME = "rs_group_queued_kernel_jit"
REF = "the built-in queued kernel field by field, bearer stores included"
VERIFIED = f"verified (8 checked calls agreed with {REF})"
_RUNS = {}


@pytest.fixture(scope="module", autouse=True)
def cache_dir(tmp_path_factory):
    """The builds of this file go to a cache directory of its own: one hiprtc run per (shape, scheduler, build)."""
    mp = pytest.MonkeyPatch()
    d = tmp_path_factory.mktemp("queued_builds")
    mp.setenv("RS_JIT_CACHE_DIR", str(d))
    for k in ("RS_JIT_CACHE", "RS_JIT_EXTRA", "RS_JIT_LEAN", "RS_DROPIN_SELFCHECK_CALLS", "RS_JIT_SELFCHECK"):
        mp.delenv(k, raising=False)
    yield d
    mp.undo()


def _run(oracle, sched, **kw):
    key = (sched, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _RUNS:
        _RUNS[key] = oracle_run(oracle, sched, **kw)
    return _RUNS[key]


def _same_results(res, want, what):
    for f in FIELDS:
        assert BITS(getattr(res, f)) == BITS(getattr(want, f)), f"{what}: {f}"


def _same_state(g, ref, cells, what):
    for k in cells:
        (a, p, l), (ra, rp, rl) = g.get_bearers(k), ref.get_bearers(k)
        assert BITS(a) == BITS(ra), f"{what}, cell {k}: avg"
        assert BITS(p) == BITS(rp), f"{what}, cell {k}: pending_bytes"
        assert l == rl, f"{what}, cell {k}: last_update"
        assert BITS(g.slice_offset(k)) == BITS(ref.slice_offset(k)), f"{what}, cell {k}: slice offsets"


def _both(g, ref, calls, now, cell_ids=None, what="", jit=True, state=True):
    """One queued call on the specialised group and on its unspecialised twin: outputs, served-by name, and (state) the bearers."""
    res, want = g.schedule_tti_queued(calls, now, cell_ids=cell_ids), ref.schedule_tti_queued(calls, now, cell_ids=cell_ids)
    for j in range(len(calls)):
        _same_results(res[j], want[j], f"{what} slot {j}")
    assert g.kernel_name == (JIT_NAME if jit else ref.kernel_name), (g.kernel_name, g.queued_jit_status())
    if state:
        _same_state(g, ref, range(g.n_cells) if cell_ids is None else cell_ids, what)
    return res


def _drive(g, ref, run, sched, what, permute=False, state_every=False):
    """oracle_run's steps through both groups; permute: odd TTIs name the cells in reverse order."""
    K, U = len(run["kinds"]), len(run["kinds"][0])
    for k in range(K):
        for grp in (g, ref):
            grp.set_bearers(k, run["kinds"][k] != 0, np.full((U, 2), 100000.0), 0.1)
    for t, row in enumerate(run["steps"]):
        calls, ids = device_calls(sched, row), None
        if permute and t % 2:
            ids = list(range(K))[::-1]
            calls = [calls[k] for k in ids]
        _both(g, ref, calls, run["ticks"][t], cell_ids=ids, what=f"{what} TTI {t}", state=state_every or (t + 1) in run["state"])
    assert g.launch_count == ref.launch_count == len(run["steps"])  # the twin launch of a checked call is not counted


# ---------------------------------------------------------------------------------------------------------------------------
# 1. equal to the built-in queued kernel
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("selfcheck", ["2", "0"])
@pytest.mark.parametrize("sched", [8, 9, 7, 103])
def test_equal_to_the_built_in_queued_kernel(rs, oracle, sched, selfcheck, monkeypatch):
    monkeypatch.setenv("RS_JIT_SELFCHECK", selfcheck)
    run = _run(oracle, sched)
    ref = make_group(rs, sched)
    g = make_group(rs, sched)
    g.specialize_queued()
    assert g.queued_jit_status()[0] == 1 and g.jit_status()[0] == 0 and g.resident_jit_status()[0] == 0, g.queued_jit_status()
    _drive(g, ref, run, sched, f"sched {sched}")
    assert set(run["state"]) == set(STATE_AT)
    code, msg = g.queued_jit_status()
    assert code == 1, (code, msg)
    # (scheduler 7's calls carry required_rbs, the gate: the general build serves them; the others' calls are plain)
    served, other = ("general", "lean") if sched == 7 else ("lean", "general")
    if selfcheck == "2":
        assert f"{served} build: {VERIFIED}" in msg and f"{other} build: 0 checked call(s) agreed" in msg, msg
    else:
        assert "agreed" not in msg, msg
    g.close()
    ref.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. against the oracle's DoSchedule() with queues
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sched", [8, 9, 7, 103])
def test_specialised_queued_calls_against_the_oracle(rs, oracle, sched, monkeypatch):
    monkeypatch.setenv("RS_JIT_SELFCHECK", "2")
    run = _run(oracle, sched)
    n = binding_counts(run)   # from the scenario alone: what the builds are pinned on
    assert n["both"] > 0, "no slot in which a user had data in both bearers"
    assert n["less"] > 0 and n["split"] > 0, "no grant exceeded a bearer's queue"
    if sched != 7:  # (scheduler 7's slices always hold an InfiniteBuffer bearer: its cells never fall idle)
        assert n["idle"] > 0, "no update-only slot"
        first8 = [[len(st["ids"]) == 0 for st in row] for row in run["steps"][:8]]
        assert any(any(r) and not all(r) for r in first8), "no mixed call among the checked ones"
    g = make_group(rs, sched)
    g.specialize_queued()
    follow_the_oracle(g, run, sched, f"specialised, sched {sched}")
    assert g.kernel_name == JIT_NAME
    code, msg = g.queued_jit_status()
    assert code == 1 and VERIFIED in msg, (code, msg)
    g.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the general build's paths
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
    """Customised slices (algo_alpha = 1, hol_delay, prio_has_data), per-PRB reports, scheduler 7's required_rbs: 5 such calls, then 3
    plain ones.  The lean build serves none of the former and all of the latter -- but a config with customised slices has no plain call."""
    monkeypatch.setenv("RS_JIT_SELFCHECK", "2")
    cfg = dict(algo_alpha=[1, 1, 1], algo_beta=[1, 1, 1]) if variant == "custom" else {}
    ref, g = make_group(rs, sched, **cfg), make_group(rs, sched, **cfg)
    g.specialize_queued()
    rng = np.random.default_rng(300 + sched + len(variant))
    has, avg = _bearers(rng)
    for k in range(CELLS):
        for grp in (g, ref):
            grp.set_bearers(k, has[k], avg[k], 0.1)
    for t in range(5):
        _both(g, ref, _random_calls(rng, has, t, sched, variant, 3000), 0.101 + 0.001 * t, what=f"{variant} call {t}")
    code, msg = g.queued_jit_status()
    assert code == 1 and f"general build: 5 checked call(s) agreed with {REF}, 3 to go" in msg and "lean build: 0 checked call(s) agreed" in msg, msg
    for t in range(5, 8):
        _both(g, ref, _random_calls(rng, has, t, sched, "custom" if variant == "custom" else None, 3000), 0.101 + 0.001 * t, what=f"plain call {t}")
    code, msg = g.queued_jit_status()
    if variant == "custom":
        assert code == 1 and f"general build: {VERIFIED}" in msg and "lean build: 0 checked call(s) agreed" in msg, msg
    else:
        assert code == 1 and "general build: 5 checked call(s) agreed" in msg and "lean build: 3 checked call(s) agreed" in msg, msg
    assert g.launch_count == ref.launch_count == 8
    g.close()
    ref.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. more bearers than threads, user_id subsets, permuted cell_ids
# ---------------------------------------------------------------------------------------------------------------------------

def test_more_bearers_than_threads_and_permuted_cells(rs, oracle, monkeypatch):
    """2 x 350 users (the shape of tests/test_gpu_group_queued.py): the constant-stride update covers 1 400 bearers, gather and credit
    up to 700 call positions; every call names a user_id subset (the active users), odd TTIs name the cells in reverse order."""
    monkeypatch.setenv("RS_JIT_SELFCHECK", "2")
    kw = dict(ues=[350, 350], R=4, G=2, K=2)
    run = _run(oracle, 9, n_tti=12, grid_every=5, seed=3, busy=0.5, state_at=(1, 2, 12), **kw)
    sizes = [len(st["ids"]) for row in run["steps"] for st in row]
    assert max(sizes) > 512 and min(sizes) < 700
    ref, g = make_group(rs, 9, **kw), make_group(rs, 9, **kw)
    g.specialize_queued()
    _drive(g, ref, run, 9, "700 users", permute=True, state_every=True)
    code, msg = g.queued_jit_status()
    assert code == 1 and f"lean build: {VERIFIED}" in msg, (code, msg)
    g.close()
    ref.close()
    g = make_group(rs, 9, **kw)   # ... and the same builds (marked by now, checked again) against the oracle
    g.specialize_queued()
    follow_the_oracle(g, run, 9, "700 users, specialised")
    assert g.kernel_name == JIT_NAME
    g.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. update-only launches
# ---------------------------------------------------------------------------------------------------------------------------

def test_update_only_launches(rs, monkeypatch):
    monkeypatch.setenv("RS_JIT_SELFCHECK", "2")
    ref, g = make_group(rs, 9), make_group(rs, 9)
    g.specialize_queued()
    rng = np.random.default_rng(7)
    has = np.ones((U_ALL, 2), bool)
    has[3] = (True, False)
    for k in range(CELLS):
        for grp in (g, ref):
            grp.set_bearers(k, has, np.full((U_ALL, 2), 2e5), 0.1)
    every = range(CELLS)
    _both(g, ref, [simple_call(rng, 70 + k, n=U_ALL) for k in every], 0.101, what="full call")
    assert all(g.get_bearers(k)[1].any() for k in every)
    # a mixed call inside the checked ones: cell 1 has nobody to schedule
    res = _both(g, ref, [simple_call(rng, 80, n=U_ALL), dict(n_users=0), simple_call(rng, 82, n=U_ALL)], 0.102, what="mixed call")
    assert (res[1].rbg_to_user == -1).all() and not res[1].target_rbs.any() and (res[0].rbg_to_user >= 0).any()
    assert not g.get_bearers(1)[1].any() and g.get_bearers(1)[2] == 0.102
    # empty slots only, named out of order, a clock per cell: one launch, a checked call like any other
    _both(g, ref, [dict(n_users=0)] * CELLS, [0.103, 0.104, 0.105], cell_ids=[2, 0, 1], what="empty slots only")
    assert [g.get_bearers(k)[2] for k in every] == [0.104, 0.105, 0.103]
    assert not any(g.get_bearers(k)[1].any() for k in every)
    _both(g, ref, [dict(n_users=0)], [0.104], cell_ids=[0], what="the same clock again")
    _both(g, ref, [simple_call(rng, 90 + k, n=U_ALL) for k in every], 0.106, what="full call after the empty ones")
    assert g.launch_count == ref.launch_count == 5
    code, msg = g.queued_jit_status()
    assert code == 1 and f"lean build: 5 checked call(s) agreed with {REF}, 3 to go" in msg, (code, msg)
    g.close()
    ref.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. names and independence of the three pairs; 7. a build that is wrong in its bearer stores alone
# ---------------------------------------------------------------------------------------------------------------------------

def _three_forms(rs, rng, g, ref, it, queued_jit=True, resident_jit=True):
    """A plain call on every cell, a resident call on cell 2, a queued call on cells 1 and 0: each on its own entry point."""
    plain = [dict(cqi=synth_cqi(500 + 10 * it + k, (U_ALL, R_SMALL), HIST), avg_rate=rng.uniform(1e3, 5e6, U_ALL), rand0=3 + it, rand1=4 + k)
             for k in range(CELLS)]
    for a, b in zip(g.schedule_tti(plain), ref.schedule_tti(plain)):
        _same_results(a, b, f"round {it}: plain call")
    assert g.kernel_name == "rs_group_kernel_jit"
    at = [dict(cqi=synth_cqi(600 + it, (U_ALL, R_SMALL), HIST), rand0=5 + it, rand1=6)]
    now = 0.101 + 0.001 * it
    _same_results(g.schedule_tti_at(at, now, cell_ids=[2])[0], ref.schedule_tti_at(at, now, cell_ids=[2])[0], f"round {it}: resident call")
    assert g.kernel_name == ("rs_group_resident_kernel_jit" if resident_jit else ref.kernel_name)
    assert all(BITS(x) == BITS(y) for x, y in zip(g.get_avg(2)[:2], ref.get_avg(2)[:2])), f"round {it}: resident stores"
    data = np.tile(np.array([300, 900], np.int32), (U_ALL, 1))
    _both(g, ref, [simple_call(rng, 700 + 10 * it + k, n=U_ALL, data=data) for k in range(2)], now, cell_ids=[1, 0], what=f"round {it}: queued call",
          jit=queued_jit)


def _three_pairs(rs, rng):
    ref = make_group(rs, 9)
    g = rs.GroupScheduler(rs.SliceConfig(UES), R_SMALL, G_SMALL, CELLS, sched=9, jit=True, jit_resident=True, jit_queued=True)
    a0 = rng.uniform(1e3, 5e6, U_ALL)
    for grp in (g, ref):
        for k in range(2):
            grp.set_bearers(k, np.ones((U_ALL, 2), bool), np.stack([a0, a0[::-1]], axis=1), 0.1)
        grp.set_avg(2, a0, 0.1)
    return g, ref


def test_names_and_independence_of_the_three_pairs(rs, monkeypatch):
    monkeypatch.setenv("RS_JIT_SELFCHECK", "2")
    rng = np.random.default_rng(61)
    g, ref = _three_pairs(rs, rng)
    assert (g.jit_status()[0], g.resident_jit_status()[0], g.queued_jit_status()[0]) == (1, 1, 1)
    for it in range(3):
        _three_forms(rs, rng, g, ref, it)
    assert "lean build: 3 checked call(s) agreed with the built-in kernel field by field, 5 to go" in g.jit_status()[1], g.jit_status()
    assert "lean build: 3 checked call(s) agreed with the built-in resident kernel" in g.resident_jit_status()[1], g.resident_jit_status()
    assert f"lean build: 3 checked call(s) agreed with {REF}, 5 to go" in g.queued_jit_status()[1], g.queued_jit_status()
    assert g.launch_count == 9
    stats = rs.jit_cache_stats()
    g.specialize_queued()   # RS_OK, nothing built
    assert rs.jit_cache_stats() == stats
    g.close()
    ref.close()
    # specialize_queued() later, between two calls: no state is touched; a scheduler without a queued form is refused
    g, ref = make_group(rs, 9), make_group(rs, 9)
    for grp in (g, ref):
        grp.set_bearers(0, np.ones((U_ALL, 2), bool), np.full((U_ALL, 2), 2e5), 0.1)
    _both(g, ref, [simple_call(rng, 800, n=U_ALL)], 0.101, cell_ids=[0], what="before specialize_queued", jit=False)
    before = [BITS(x) for x in g.get_bearers(0)[:2]] + [BITS(g.slice_offset(0))]
    g.specialize_queued()
    assert [BITS(x) for x in g.get_bearers(0)[:2]] + [BITS(g.slice_offset(0))] == before
    _both(g, ref, [simple_call(rng, 801, n=U_ALL)], 0.102, cell_ids=[0], what="after specialize_queued")
    g.close()
    ref.close()
    g = make_group(rs, 10)
    with pytest.raises(rs.RadioSaberError) as e:
        g.specialize_queued()
    assert e.value.code == -1 and g.queued_jit_status()[0] == 0   # RS_ERR_INVALID
    g.close()


def test_a_wrong_queued_build_is_dropped_on_state_alone(rs, monkeypatch, tmp_path):
    """-DRS_FAULT_INJECT_QUEUED: the run-time queued kernel credits one byte more to the last bearer it credits for a position (a wrong
    value, no address).  Its outputs are right; the first call's comparison of the bearer stores drops the queued pair, and it alone."""
    monkeypatch.delenv("RS_JIT_SELFCHECK", raising=False)
    monkeypatch.setenv("RS_JIT_EXTRA", "-DRS_FAULT_INJECT_QUEUED")
    monkeypatch.setenv("RS_JIT_CACHE_DIR", str(tmp_path))
    rng = np.random.default_rng(66)
    g, ref = _three_pairs(rs, rng)
    assert (g.jit_status()[0], g.resident_jit_status()[0], g.queued_jit_status()[0]) == (1, 1, 1)
    files = set(tmp_path.glob("*.rsco"))
    assert len(files) == 6
    queued_files = {f for f in files if b"-DRS_JIT_GROUP_QUEUED=1" in f.read_bytes()}
    assert len(queued_files) == 2
    _three_forms(rs, rng, g, ref, 0, queued_jit=False)   # RS_OK; outputs and bearer state: the built-in kernel's
    code, msg = g.queued_jit_status()
    assert code == -2 and "pending_bytes[" in msg and "cell " in msg and "checked call 1" in msg, (code, msg)
    assert "the built-in queued kernel serves" in msg, msg
    assert set(tmp_path.glob("*.rsco")) == files - queued_files, "the rejected queued builds are still in the cache"
    assert g.jit_status()[0] == 1 and g.resident_jit_status()[0] == 1   # the other two pairs stay
    with pytest.raises(rs.RadioSaberError) as e:
        g.specialize_queued()
    assert e.value.code == -4 and "pending_bytes[" in str(e.value)   # RS_ERR_STATE, with the reason
    for it in range(1, 4):
        _three_forms(rs, rng, g, ref, it, queued_jit=False)
        assert g.kernel_name.startswith("rs_group_queued_kernel<9,")
    assert g.launch_count == ref.launch_count == 12
    g.close()
    ref.close()
    # the reverse: a wrong RESIDENT build is dropped alone, the queued pair stays in service
    monkeypatch.setenv("RS_JIT_EXTRA", "-DRS_FAULT_INJECT_RESIDENT -DRS_BESIDE_THE_QUEUED_PAIR")  # (a key of this test's own)
    g, ref = _three_pairs(rs, rng)
    _three_forms(rs, rng, g, ref, 0, resident_jit=False)
    assert (g.jit_status()[0], g.resident_jit_status()[0], g.queued_jit_status()[0]) == (1, -2, 1)
    _three_forms(rs, rng, g, ref, 1, resident_jit=False)
    g.close()
    ref.close()
    # the same wrong queued build without the check really leaves wrong pending bytes (the injection bites)
    monkeypatch.setenv("RS_JIT_SELFCHECK", "0")
    monkeypatch.setenv("RS_JIT_EXTRA", "-DRS_FAULT_INJECT_QUEUED -DRS_UNCHECKED_TWIN")  # (another key: the first one is rejected for this process)
    g, ref = make_group(rs, 9), make_group(rs, 9)
    g.specialize_queued()
    for grp in (g, ref):
        grp.set_bearers(0, np.ones((U_ALL, 2), bool), np.full((U_ALL, 2), 2e5), 0.1)
    data = np.tile(np.array([300, 40], np.int32), (U_ALL, 1))
    _both(g, ref, [simple_call(rng, 900, n=U_ALL, data=data)], 0.101, cell_ids=[0], what="unchecked wrong build", state=False)   # the outputs are right ...
    mine, theirs = g.get_bearers(0)[1], ref.get_bearers(0)[1]
    served = theirs.any(axis=1)
    assert served.any()
    np.testing.assert_array_equal((mine - theirs).sum(axis=1), served.astype(np.int32))   # ... the pending bytes are not:
    last = np.where(theirs[:, 0] > 0, 0, 1)                                                 # a byte more on the last bearer credited
    np.testing.assert_array_equal((mine - theirs)[np.arange(U_ALL), last], served.astype(np.int32))
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
g.specialize_queued()
ref = rs.GroupScheduler(sc, R_SMALL, G_SMALL, CELLS, sched=9)
rng = np.random.default_rng(6)
has = np.ones((U, 2), bool)
for k in range(CELLS):
    a0 = rng.uniform(1e3, 5e6, (U, 2))
    g.set_bearers(k, has, a0, 0.1)
    ref.set_bearers(k, has, a0, 0.1)
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
    res, want = g.schedule_tti_queued(calls, 0.101 + 0.001 * it), ref.schedule_tti_queued(calls, 0.101 + 0.001 * it)
    names.add(g.kernel_name)
    for k in range(CELLS):
        ok &= all(np.array_equal(getattr(res[k], f), getattr(want[k], f)) for f in FIELDS)
        ok &= all(np.array_equal(a, b) for a, b in zip(g.get_bearers(k), ref.get_bearers(k)))
        ok &= g.slice_offset(k).tobytes() == ref.slice_offset(k).tobytes()
out = dict(ok=bool(ok), status=g.queued_jit_status(), others=[g.jit_status()[0], g.resident_jit_status()[0]], kernels=sorted(names),
           launches=g.launch_count, stats=rs.jit_cache_stats())
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
    assert first["ok"] and first["status"][0] == 1 and first["kernels"] == [JIT_NAME] and first["launches"] == 16 and first["others"] == [0, 0], first
    assert f"general build: {VERIFIED}" in first["status"][1] and f"lean build: {VERIFIED}" in first["status"][1], first
    marks = sorted(f.read_bytes()[-8:].decode() for f in tmp_path.glob("*.rsco"))
    assert first["stats"]["misses"] == 2 and marks == ["VERIFIED", "VERIFIED"], (first, marks)
    second = _child(tmp_path)
    assert second["ok"] and second["stats"] == {"hits": 2, "misses": 0, "stores": 0, "rejected": 0}, second
    assert second["status"][0] == 1 and second["kernels"] == [JIT_NAME] and second["launches"] == 16, second
    assert "general build: carries the self-check mark" in second["status"][1] and "lean build: carries the self-check mark" in second["status"][1], second
    assert "agreed" not in second["status"][1], second   # no call was a checked one
