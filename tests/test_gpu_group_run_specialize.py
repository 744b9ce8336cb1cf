"""rs_group_specialize_run: a group's own run-time builds of the RUN kernel (entry point rs_group_run_kernel_jit, general and lean), checked
one run at a time against the built-in run kernel on the outputs of every (cell, TTI) AND on state -- slice state, the averages and
pending bytes of every user id, the last-update time.  Against an unspecialised group for every scheduler a run serves, on the general
build's paths, against the oracle's DoSchedule loop at the small and at the sort shape, with more users than threads, beside the
resident pair of rs_group_specialize_resident, with a build that is wrong in its state alone, and with the self-check mark that travels
to the next process.  Every comparison is bitwise."""
import functools
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import synth_cqi
from test_gpu_group import HIST, _same
from test_gpu_group_run import G, K, R, RUN_SCHEDS, UES, W, _calls, _pairs, _same_runs, _state

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
JIT_NAME = "rs_group_run_kernel_jit"
RESIDENT_JIT_NAME = "rs_group_resident_kernel_jit"
REF = "the built-in run kernel field by field over every TTI, resident stores included"


def _checked(monkeypatch, calls="2"):
    """The next `calls` runs of every build are checked ones, whatever mark an earlier test left in the cache; "0": none is."""
    monkeypatch.setenv("RS_DROPIN_SELFCHECK_CALLS", calls)
    monkeypatch.setenv("RS_JIT_SELFCHECK", "2")


class _Pair:
    """An unspecialised group and one that took specialize_run(), fed the same runs: after every run every rs_tti_out field of every
    (cell, TTI) and (avg, pending, last_update, slice offsets) of EVERY cell, named or not, and image_stats must be identical."""

    def __init__(self, rs, sched, seed, ues=UES, w=W, n_rbgs=R, g_size=G, n_cells=K, **kw):
        self.rs, self.sched, self.n_cells, self.n = rs, sched, n_cells, 0
        self.sc = rs.SliceConfig(list(ues), weight=list(w))
        self.ref = rs.GroupScheduler(self.sc, n_rbgs, g_size, n_cells, sched=sched)
        self.g = rs.GroupScheduler(self.sc, n_rbgs, g_size, n_cells, sched=sched, **(kw or dict(jit_run=True)))
        self.rng = np.random.default_rng(seed)
        for k in range(n_cells):
            a0 = self.rng.uniform(1e3, 5e6, self.sc.n_users)
            for grp in (self.ref, self.g):
                grp.set_avg(k, a0, 0.1)

    def run(self, calls, nows, rands, cell_ids=None, served_by_jit=True):
        res = self.g.run_at(calls, nows, rands, cell_ids=cell_ids)
        want = self.ref.run_at(calls, nows, rands, cell_ids=cell_ids)
        self.n += 1
        what = f"sched {self.sched} call {self.n}"
        _same_runs(res, want, what, upper=self.sched == 10)
        self.same_state(what)
        assert self.g.kernel_name == (JIT_NAME if served_by_jit else self.ref.kernel_name), (self.g.kernel_name, self.g.run_jit_status())
        assert self.ref.kernel_name.startswith(f"rs_group_run_kernel<{self.sched},")
        return res

    def at(self, calls, now, served_by_jit):
        res, want = self.g.schedule_tti_at(calls, now), self.ref.schedule_tti_at(calls, now)
        self.n += 1
        for k in range(len(calls)):
            _same(res[k], want[k], f"sched {self.sched} call {self.n} (at) slot {k}", upper=self.sched == 10)
        self.same_state(f"sched {self.sched} call {self.n} (at)")
        assert self.g.kernel_name == (RESIDENT_JIT_NAME if served_by_jit else self.ref.kernel_name), (self.g.kernel_name, self.g.resident_jit_status())

    def same_state(self, what):
        assert _state(self.g, self.n_cells) == _state(self.ref, self.n_cells), f"{what}: avg / pending_bytes / last_update / slice offsets"
        assert self.g.image_stats == self.ref.image_stats, f"{what}: image_stats"

    def close(self):
        self.g.close()
        self.ref.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 1. equal to the built-in run kernel, every scheduler of a run, checked and unchecked
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("calls", ["2", "0"])
@pytest.mark.parametrize("T", [1, 2, 7])
@pytest.mark.parametrize("sched", RUN_SCHEDS)
def test_equal_to_the_built_in_run_kernel(rs, sched, T, calls, monkeypatch):
    """Three runs in a row, new grids and a new cqi_epoch before each.  RS_DROPIN_SELFCHECK_CALLS=2: the first two runs are checked ones;
    =0: none is."""
    _checked(monkeypatch, calls)
    p = _Pair(rs, sched, 100 * sched + T)
    assert p.g.run_jit_status()[0] == 1 and p.g.resident_jit_status()[0] == 0 and p.g.jit_status()[0] == 0, p.g.run_jit_status()
    now = 0.1
    for run in range(3):
        cs = _calls(K, p.sc.n_users, 2000 * sched + 10 * run + T, epoch=1 + run)
        nows = now + 0.001 * np.arange(1, T + 1)
        now = float(nows[-1])
        p.run(cs, nows, _pairs(p.rng, K, T))
        assert p.g.get_avg(0)[2] == now
        assert p.g.image_stats == ((run + 1) * K * (T - 1), (run + 1) * K, 0)   # a checked run is counted once
    assert p.g.launch_count == 3 and p.ref.launch_count == 3   # the twin launch of a checked run is not counted
    code, msg = p.g.run_jit_status()
    assert code == 1, (code, msg)
    # (scheduler 10 through this wrapper always asks for the upper_* lists, which the lean build does not write: the general build serves)
    served, other = ("general", "lean") if sched == 10 else ("lean", "general")
    if calls == "2":
        assert f"{served} build: verified (2 checked calls agreed with {REF})" in msg and f"{other} build: 0 checked call(s) agreed" in msg, msg
    else:
        assert "agreed" not in msg, msg
    p.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the general build's paths
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant,lean", [("prb", "0"), ("subset", "0"), ("subset", "1"), ("cells", "0"), ("cells", "1"),
                                          ("epoch 0", "0"), ("epoch 0", "1"), ("clock", "0"), ("clock", "1")])
def test_general_build_paths(rs, variant, lean, monkeypatch):
    """Per-PRB reports under a number (TTI 0 writes the cell's store, the later TTIs and the second run read it), a user_id subset of
    the cells' users, cell_ids naming 2 of the 3 cells, a run without cqi_epoch (every TTI reads the slot's block again), a clock step
    of 0 inside the run.  RS_JIT_LEAN=0: the general build serves every one of them; =1: it serves the per-PRB runs, the lean build the
    others (so the per-PRB variant has the one case).  Two runs each, both checked."""
    _checked(monkeypatch)
    monkeypatch.setenv("RS_JIT_LEAN", lean)
    p = _Pair(rs, 9, 200 + len(variant))
    U, T = p.sc.n_users, 4
    cell_ids, n = ([2, 0], 2) if variant == "cells" else (None, K)
    ids = np.array([0, 2, 3, 5, 8, 9, 11], np.int32)
    now = 0.1
    for run in range(2):
        if variant == "prb":
            cs = [dict(cqi_prb=synth_cqi(2200 + k, (U, R * G), HIST), cqi_epoch=9) for k in range(n)]   # the second run repeats the number
        elif variant == "subset":
            cs = [dict(cqi=synth_cqi(2300 + 10 * run + k, (len(ids), R), HIST), user_id=ids, cqi_epoch=3 + run) for k in range(n)]
        else:
            cs = _calls(n, U, 2400 + 10 * run, epoch=0 if variant == "epoch 0" else 5 + run)
        nows = now + (np.array([0.001, 0.002, 0.002, 0.003]) if variant == "clock" else 0.001 * np.arange(1, T + 1))
        now = float(nows[-1])
        p.run(cs, nows, _pairs(p.rng, n, T), cell_ids=cell_ids)
    if variant == "epoch 0":
        assert p.g.image_stats == (0, 0, 2 * T * K)
    elif variant == "prb":
        assert p.g.image_stats == ((2 * T - 1) * K, K, 0)
    code, msg = p.g.run_jit_status()
    served = "general" if (variant == "prb" or lean == "0") else "lean"
    assert code == 1 and f"{served} build: verified (2 checked calls agreed with {REF})" in msg, (code, msg)
    assert ("lean build: not built" in msg) == (lean == "0"), msg
    assert p.g.launch_count == 2
    p.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. against the oracle's own DoSchedule loop
# ---------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _oracle_runs(sched, ues, w, n_rbgs, g_size, n_cells, n_runs, T, seed):
    """The oracle's side, computed once per case: per run the grids, the clock and the rand() pairs the run is given, the oracle's
    outputs per (cell, TTI), its averages and slice state behind the run; and the starting averages."""
    from oracle import oracle_py as oracle
    U = sum(ues)
    cells = [oracle.Cell(list(ues), n_rbgs, g_size, sched, weights=list(w)) for _ in range(n_cells)]
    ticks = oracle.clock_ticks(100, n_runs * T)
    rngs = [oracle.Rng(seed + 17 * k) for k in range(n_cells)]
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
        runs.append(dict(grids=grids, nows=nows, rands=pairs, outs=outs, avg=[cells[k].state()["avg_rate"].copy() for k in range(n_cells)],
                         slices=[cells[k].state()["slice_state"].copy() for k in range(n_cells)]))
    return a0, runs


@pytest.mark.parametrize("shape", ["small", "sort"])
def test_against_the_oracle(rs, oracle, shape, monkeypatch):
    """Scheduler 9, two runs of T = 5 on the clock of the oracle's run loops, both checked: every rs_tti_out field of every TTI, the
    averages and the slice offsets behind each run.  small: 3 cells, slices of 5 / 4 / 3 users, 8 RBGs of 2; sort: 2 cells, 20 slices
    x 5 users, 64 RBGs of 8 (1 280 sort records on 512 threads)."""
    _checked(monkeypatch)
    ues, w, n_rbgs, g_size, n_cells = (UES, W, R, G, K) if shape == "small" else ([5] * 20, [0.05] * 20, 64, 8, 2)
    n_runs, T = 2, 5
    a0, runs = _oracle_runs(9, tuple(ues), tuple(w), n_rbgs, g_size, n_cells, n_runs, T, 7400 + len(shape))
    sc = rs.SliceConfig(list(ues), weight=list(w))
    g = rs.GroupScheduler(sc, n_rbgs, g_size, n_cells, sched=9, jit_run=True)
    for k in range(n_cells):
        g.set_avg(k, a0[k], 0.1)
    for i, run in enumerate(runs):
        res = g.run_at([dict(cqi=run["grids"][k], cqi_epoch=1 + i) for k in range(n_cells)], run["nows"], run["rands"])
        assert g.kernel_name == JIT_NAME, g.run_jit_status()
        for k in range(n_cells):
            for t in range(T):
                _same(res[k][t], run["outs"][k][t], f"{shape} run {i} cell {k} TTI {t}")
            a, _, last = g.get_avg(k)
            assert a.tobytes() == run["avg"][k].tobytes(), f"{shape} after run {i}, cell {k}: averages"
            assert last == run["nows"][-1]
            assert g.slice_offset(k).tobytes() == run["slices"][k].tobytes(), f"{shape} after run {i}, cell {k}: slice offsets"
    code, msg = g.run_jit_status()
    assert code == 1 and f"lean build: verified (2 checked calls agreed with {REF})" in msg, (code, msg)
    assert g.launch_count == n_runs and g.image_stats == (n_runs * n_cells * (T - 1), n_runs * n_cells, 0)
    g.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. more users than threads
# ---------------------------------------------------------------------------------------------------------------------------

def test_more_users_than_threads(rs, monkeypatch):
    """7 slices x 100 users, 25 RBGs of 4, one cell, one checked run of T = 2 with a user_id list of 600 users: the RS_JIT_NT-strided
    update, gather and credit loops of the run-time build run more than once per thread (at most 512 threads) in both TTIs."""
    _checked(monkeypatch)
    p = _Pair(rs, 9, 44, ues=[100] * 7, w=[1.0 / 7] * 7, n_rbgs=25, g_size=4, n_cells=1)
    U = p.sc.n_users
    a0 = p.g.get_avg(0)[0]
    ids = np.sort(p.rng.choice(U, 600, replace=False)).astype(np.int32)
    nows = np.array([0.101, 0.102])
    p.run([dict(cqi=synth_cqi(4400, (len(ids), 25), HIST), user_id=ids, cqi_epoch=1)], nows, _pairs(p.rng, 1, 2))
    a, pend, last = p.g.get_avg(0)
    assert last == 0.102 and np.count_nonzero(pend) > 0 and not np.count_nonzero(pend[np.setdiff1d(np.arange(U), ids)])
    assert (a != a0).all()   # every one of the 700 was updated
    code, msg = p.g.run_jit_status()
    assert code == 1 and "lean build: 1 checked call(s) agreed" in msg, (code, msg)
    p.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. independence of the pairs
# ---------------------------------------------------------------------------------------------------------------------------

def test_independence_of_the_resident_and_the_run_pair(rs, monkeypatch):
    _checked(monkeypatch, "8")
    T = 3
    nows = lambda now: now + 0.001 * np.arange(1, T + 1)   # noqa: E731
    at_calls = lambda p, seed, epoch: [dict(c, rand0=5, rand1=6) for c in _calls(K, p.sc.n_users, seed, epoch=epoch)]   # noqa: E731
    # specialize_resident() alone: runs stay on the built-in run kernel
    p = _Pair(rs, 9, 5, jit_resident=True)
    p.run(_calls(K, p.sc.n_users, 500, epoch=1), nows(0.1), _pairs(p.rng, K, T), served_by_jit=False)
    p.at(at_calls(p, 510, 2), 0.104, served_by_jit=True)
    assert p.g.run_jit_status()[0] == 0 and p.g.resident_jit_status()[0] == 1
    p.close()
    # specialize_run() alone: at-calls stay on the built-in resident kernel
    p = _Pair(rs, 9, 6)
    p.at(at_calls(p, 520, 1), 0.101, served_by_jit=False)
    p.run(_calls(K, p.sc.n_users, 530, epoch=2), nows(0.101), _pairs(p.rng, K, T))
    p.at(at_calls(p, 540, 3), 0.105, served_by_jit=False)
    assert p.g.run_jit_status()[0] == 1 and p.g.resident_jit_status()[0] == 0 and p.g.jit_status()[0] == 0
    assert "lean build: 1 checked call(s) agreed" in p.g.run_jit_status()[1]
    stats = rs.jit_cache_stats()
    p.g.specialize_run()   # RS_OK, nothing built
    assert rs.jit_cache_stats() == stats
    p.close()
    # both: at-call / run / at-call equals the twin's, the name alternates, each status reports its own pair
    p = _Pair(rs, 9, 7, jit_resident=True, jit_run=True)
    assert p.g.run_jit_status()[0] == 1 and p.g.resident_jit_status()[0] == 1
    p.at(at_calls(p, 550, 1), 0.101, served_by_jit=True)
    p.run(_calls(K, p.sc.n_users, 560, epoch=2), nows(0.101), _pairs(p.rng, K, T))
    p.at(at_calls(p, 570, 3), 0.105, served_by_jit=True)
    p.run(_calls(K, p.sc.n_users, 580, epoch=4), nows(0.105), _pairs(p.rng, K, T))
    assert f"lean build: 2 checked call(s) agreed with {REF}, 6 to go" in p.g.run_jit_status()[1], p.g.run_jit_status()
    assert "lean build: 2 checked call(s) agreed with the built-in resident kernel field by field, resident stores included, 6 to go" in \
        p.g.resident_jit_status()[1], p.g.resident_jit_status()
    assert p.g.launch_count == 4
    p.close()
    # specialize_resident() first, specialize_run() later, between two calls: no state moves
    p = _Pair(rs, 9, 8, jit_resident=True)
    p.run(_calls(K, p.sc.n_users, 590, epoch=1), nows(0.1), _pairs(p.rng, K, T), served_by_jit=False)
    before = _state(p.g, K)
    p.g.specialize_run()
    assert _state(p.g, K) == before
    p.run(_calls(K, p.sc.n_users, 600, epoch=2), nows(0.103), _pairs(p.rng, K, T))
    p.close()


def test_refusals_of_configs_and_schedulers(rs):
    """What no run serves has no run builds: RS_SCHED_NVS and a config with a customised slice are RS_ERR_INVALID, nothing is built and
    the pair stays "not asked for"; the other pairs of such a group are not affected."""
    for frag, kw, sched in (("scheduler 7", {}, 7), ("algo_alpha", dict(algo_alpha=[1, 0, 0], algo_beta=[0, 0, 0]), 9)):
        sc = rs.SliceConfig(UES, weight=W, **kw)
        g = rs.GroupScheduler(sc, R, G, 1, sched=sched)
        stats = rs.jit_cache_stats()
        with pytest.raises(rs.RadioSaberError) as e:
            g.specialize_run()
        assert e.value.code == -1 and frag in str(e.value) and "rs_group_specialize_run" in str(e.value), str(e.value)
        assert rs.jit_cache_stats() == stats and g.run_jit_status()[0] == 0 and g.launch_count == 0
        g.specialize_resident()
        assert g.resident_jit_status()[0] == 1 and g.run_jit_status()[0] == 0
        g.close()
        with pytest.raises(rs.RadioSaberError):
            rs.GroupScheduler(sc, R, G, 1, sched=sched, jit_run=True)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. a build that is wrong in its state alone
# ---------------------------------------------------------------------------------------------------------------------------

def test_a_wrong_run_build_is_dropped_on_state_alone(rs, monkeypatch, tmp_path):
    """-DRS_FAULT_INJECT_RUN: in the LAST TTI of a run the run-time kernel credits every served user one byte more (a wrong value, no
    address, not T).  The outputs of all T TTIs are right; the first run's comparison of the resident stores drops the run pair."""
    monkeypatch.delenv("RS_JIT_SELFCHECK", raising=False)
    monkeypatch.delenv("RS_DROPIN_SELFCHECK_CALLS", raising=False)
    monkeypatch.setenv("RS_JIT_EXTRA", "-DRS_FAULT_INJECT_RUN")
    monkeypatch.setenv("RS_JIT_CACHE_DIR", str(tmp_path))
    T = 3
    p = _Pair(rs, 9, 66, jit_resident=True, jit_run=True)
    U = p.sc.n_users
    assert p.g.run_jit_status()[0] == 1 and p.g.resident_jit_status()[0] == 1
    files = set(tmp_path.glob("*.rsco"))
    assert len(files) == 4
    run_files = {f for f in files if b"-DRS_JIT_GROUP_RUN=1" in f.read_bytes()}
    assert len(run_files) == 2
    p.run(_calls(K, U, 6600, epoch=1), 0.1 + 0.001 * np.arange(1, T + 1), _pairs(p.rng, K, T), served_by_jit=False)   # outputs and state: the built-in kernel's
    code, msg = p.g.run_jit_status()
    assert code == -2 and "pending_bytes[" in msg and "cell " in msg and "checked call 1" in msg, (code, msg)
    assert "the built-in run kernel serves this group's runs" in msg and "run lean build" in msg, msg
    assert set(tmp_path.glob("*.rsco")) == files - run_files, "the rejected run builds are still in the cache"
    with pytest.raises(rs.RadioSaberError) as e:
        p.g.specialize_run()
    assert e.value.code == -4 and "pending_bytes[" in str(e.value)   # RS_ERR_STATE, with the reason
    now = 0.1 + 0.001 * T
    for it in range(1, 4):
        nows = now + 0.001 * np.arange(1, T + 1)
        now = float(nows[-1])
        p.run(_calls(K, U, 6600 + 10 * it, epoch=1 + it), nows, _pairs(p.rng, K, T), served_by_jit=False)
    assert p.g.launch_count == 4
    # the resident pair built beside it is still in service
    p.at([dict(c, rand0=3, rand1=4) for c in _calls(K, U, 6700, epoch=9)], now + 0.001, served_by_jit=True)
    assert p.g.resident_jit_status()[0] == 1
    p.close()
    # the same wrong build without the check really leaves wrong pending bytes -- of the last TTI alone (the injection bites)
    monkeypatch.setenv("RS_JIT_SELFCHECK", "0")
    monkeypatch.setenv("RS_JIT_EXTRA", "-DRS_FAULT_INJECT_RUN -DRS_UNCHECKED_TWIN")  # (another key: the first one is rejected for this process)
    p = _Pair(rs, 9, 67)
    cs, nows, rands = _calls(K, U, 6800, epoch=1), 0.1 + 0.001 * np.arange(1, T + 1), _pairs(p.rng, K, T)
    res, want = p.g.run_at(cs, nows, rands), p.ref.run_at(cs, nows, rands)
    assert p.g.kernel_name == JIT_NAME
    _same_runs(res, want, "unchecked wrong build")   # the outputs of all T TTIs are right ...
    for k in range(K):
        (a, mine, last), (b, theirs, last2) = p.g.get_avg(k), p.ref.get_avg(k)
        served = theirs != 0
        assert served.any() and a.tobytes() == b.tobytes() and last == last2   # (the averages saw the right bytes of TTIs 0 .. T-2)
        np.testing.assert_array_equal(mine, theirs + served)                     # ... the pending bytes behind the last TTI are not
    p.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 7. the mark travels
# ---------------------------------------------------------------------------------------------------------------------------

CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(root)r + "/tests")
import numpy as np
import radiosaber_amd as rs
from conftest import synth_cqi
from test_gpu_group import FIELDS
HIST = %(hist)r
ues, R, G, K, T = [5, 4, 3], 8, 2, 3, 2
U = sum(ues)
sc = rs.SliceConfig(ues, weight=[0.5, 0.3, 0.2])
g = rs.GroupScheduler(sc, R, G, K, sched=9)
g.specialize_run()
ref = rs.GroupScheduler(sc, R, G, K, sched=9)
rng = np.random.default_rng(6)
for k in range(K):
    a0 = rng.uniform(1e3, 5e6, U)
    g.set_avg(k, a0, 0.1)
    ref.set_avg(k, a0, 0.1)
ok, names = True, set()
for it in range(16):   # 8 plain runs (the lean build), 8 with per-PRB reports (the general build)
    calls = []
    for k in range(K):
        cqi = synth_cqi(600 + 10 * it + k, (U, R), HIST)
        kw = dict(cqi=cqi)
        if it >= 8:
            kw = dict(cqi_prb=np.repeat(cqi, G, axis=1))
        calls.append(kw)
    nows = 0.1 + 0.001 * (T * it + np.arange(1, T + 1))
    rands = rng.integers(0, 2**31 - 1, (K, T, 2)).astype(np.int32)
    res, want = g.run_at(calls, nows, rands), ref.run_at(calls, nows, rands)
    names.add(g.kernel_name)
    for k in range(K):
        for t in range(T):
            ok &= all(np.array_equal(getattr(res[k][t], f), getattr(want[k][t], f)) for f in FIELDS)
        ok &= all(np.array_equal(a, b) for a, b in zip(g.get_avg(k), ref.get_avg(k)))
        ok &= g.slice_offset(k).tobytes() == ref.slice_offset(k).tobytes()
out = dict(ok=bool(ok), status=g.run_jit_status(), resident=g.resident_jit_status()[0], kernels=sorted(names), launches=g.launch_count,
           stats=rs.jit_cache_stats())
g.close()
ref.close()
print(json.dumps(out))
"""


def _child(cache_dir):
    env = dict(os.environ, RS_JIT_CACHE_DIR=str(cache_dir), AMD_COMGR_CACHE="0")
    for k in ("RS_JIT_CACHE", "RS_JIT_SELFCHECK", "RS_JIT_EXTRA", "RS_JIT_LEAN", "RS_DROPIN_SELFCHECK_CALLS"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": str(ROOT), "hist": HIST}], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().split("\n")[-1])


def test_the_self_check_mark_travels_to_the_next_process(rs, tmp_path):
    verified = f"verified (8 checked calls agreed with {REF})"
    first = _child(tmp_path)
    assert first["ok"] and first["status"][0] == 1 and first["kernels"] == [JIT_NAME] and first["launches"] == 16 and first["resident"] == 0, first
    assert f"general build: {verified}" in first["status"][1] and f"lean build: {verified}" in first["status"][1], first
    marks = sorted(f.read_bytes()[-8:].decode() for f in tmp_path.glob("*.rsco"))
    assert first["stats"]["misses"] == 2 and marks == ["VERIFIED", "VERIFIED"], (first, marks)
    second = _child(tmp_path)
    assert second["ok"] and second["stats"] == {"hits": 2, "misses": 0, "stores": 0, "rejected": 0}, second
    assert second["status"][0] == 1 and second["kernels"] == [JIT_NAME] and second["launches"] == 16, second
    assert "general build: carries the self-check mark" in second["status"][1] and "lean build: carries the self-check mark" in second["status"][1], second
    assert "agreed" not in second["status"][1], second   # no run was a checked one
