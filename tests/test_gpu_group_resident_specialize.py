"""rs_group_specialize_resident: a group's own run-time builds of the RESIDENT kernel (entry point rs_group_resident_kernel_jit, general
and lean), checked against the built-in resident kernel on outputs AND on state -- slice state, the averages of every user id, the
pending bytes, the last-update time.  Against an unspecialised group for every scheduler, on the general build's paths, against the
oracle's DoSchedule loop at the sort shape, with more users than threads, beside the plain pair of rs_group_specialize, with a build
that is wrong in its state alone, and with the self-check mark that travels to the next process.  Every comparison is bitwise."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import synth_cqi
import test_gpu_group_resident as small   # its shape (slices of 5 / 4 / 3 users, 8 RBGs of 2) is the one _plain_calls deals
from test_gpu_group import HIST, SCHEDS
from test_gpu_group_resident import _plain_calls, _same, _state, _update

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
UES, R, G, K = [3, 4, 0, 2, 5], 12, 2, 3      # ragged slices, an empty slice; 12 RBGs of 2 PRBs; 3 cells
W = [0.3, 0.2, 0.1, 0.15, 0.25]
JIT_NAME = "rs_group_resident_kernel_jit"
REF = "the built-in resident kernel field by field, resident stores included"
VERIFIED = f"verified (8 checked calls agreed with {REF})"


def _rand2(rng):
    return int(rng.integers(0, 2**31 - 1)), int(rng.integers(0, 2**31 - 1))


def _calls(rng, sc, sched, n_rbgs, cells, seed, epoch=0, subset=False, pick=0, variant=None):
    """One resident call's keyword dictionaries for `cells`: all users or (subset) ascending per-cell user_id lists -- scheduler 7 always
    names the users of one slice, slice number `pick` + cell of the non-empty ones --, per-cell grids and rand() pairs, the variant's
    optional inputs.  `pick` and `seed` fix the lists: a call that repeats them under the same cqi_epoch is served from the cell's image."""
    U, u2s = sc.n_users, np.asarray(sc.user_to_slice)
    live = [s for s in range(sc.n_slices) if (u2s == s).any()]
    ids_rng = np.random.default_rng(seed)
    calls = []
    for k in cells:
        ids = None
        if sched == 7:
            ids = np.flatnonzero(u2s == live[(k + pick) % len(live)]).astype(np.int32)
        elif subset:
            ids = np.sort(ids_rng.choice(U, int(ids_rng.integers(1, U)), replace=False)).astype(np.int32)
        n = U if ids is None else len(ids)
        cqi = synth_cqi(seed * 131 + k, (n, n_rbgs), HIST)
        r0, r1 = _rand2(rng)
        kw = dict(cqi=cqi, rand0=r0, rand1=r1, cqi_epoch=epoch)
        if ids is not None:
            kw["user_id"] = ids
        if variant == "prb":
            prb = np.repeat(cqi, G, axis=1)
            prb[:, 1::G] = np.maximum(1, prb[:, 1::G] - 1)
            kw["cqi"], kw["cqi_prb"] = None, prb
        if variant == "custom":
            kw["hol_delay"] = rng.uniform(1e-5, 0.3, n)
            kw["prio_has_data"] = (rng.random(n) < 0.8).astype(np.uint8)
        if variant == "gates":
            kw["required_rbs"] = rng.integers(0, 3 * G, n).astype(np.int32)
        calls.append(kw)
    return calls


class _Pair:
    """An unspecialised group and one that took specialize_resident(), fed the same resident calls: after every call every rs_tti_out
    field of the named cells and (avg, pending, last_update, slice offsets) of EVERY cell, named or not, must be identical."""

    def __init__(self, rs, sc, n_rbgs, n_cells, sched, seed, both=False):
        self.rs, self.sched, self.n_cells, self.n = rs, sched, n_cells, 0
        self.ref = rs.GroupScheduler(sc, n_rbgs, G, n_cells, sched=sched)
        self.g = rs.GroupScheduler(sc, n_rbgs, G, n_cells, sched=sched, jit=both, jit_resident=True)
        rng = np.random.default_rng(seed)
        for k in range(n_cells):
            a0 = rng.uniform(1e3, 5e6, sc.n_users)
            for grp in (self.ref, self.g):
                grp.set_avg(k, a0, 0.1)

    def call(self, calls, now, cell_ids=None, served_by_jit=True):
        res = self.g.schedule_tti_at(calls, now, cell_ids=cell_ids)
        want = self.ref.schedule_tti_at(calls, now, cell_ids=cell_ids)
        self.n += 1
        for j in range(len(calls)):
            _same(res[j], want[j], f"sched {self.sched} call {self.n} slot {j}", upper=self.sched == 10)
        self.same_state(f"sched {self.sched} after call {self.n}")
        assert self.g.kernel_name == (JIT_NAME if served_by_jit else self.ref.kernel_name), (self.g.kernel_name, self.g.resident_jit_status())
        return res

    def same_state(self, what):
        mine, theirs = _state(self.g, self.n_cells), _state(self.ref, self.n_cells)
        for k in range(self.n_cells):
            for name, a, b in zip(("avg", "pending_bytes", "last_update"), mine[k], theirs[k]):
                assert a == b, f"{what}, cell {k}: {name}"
            assert self.g.slice_offset(k).tobytes() == self.ref.slice_offset(k).tobytes(), f"{what}, cell {k}: slice offsets"

    def close(self):
        self.g.close()
        self.ref.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 1. equal to the built-in resident kernel, every scheduler, checked and unchecked
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("selfcheck", ["2", "0"])
@pytest.mark.parametrize("sched", SCHEDS)
def test_equal_to_the_built_in_resident_kernel(rs, sched, selfcheck, monkeypatch):
    """12 resident calls: all users and user_id subsets, cell subsets and permutations, one call with now == last_update, a clock per
    cell, cqi_epoch in all three modes (none, stored, served from the image -- mixed inside one launch).  RS_JIT_SELFCHECK=2: the
    first 8 calls of the serving build are checked ones; =0: none is."""
    monkeypatch.setenv("RS_JIT_SELFCHECK", selfcheck)
    sc = rs.SliceConfig(UES, weight=W)
    p = _Pair(rs, sc, R, K, sched, seed=40 + sched)
    assert p.g.resident_jit_status()[0] == 1 and p.g.jit_status()[0] == 0, (p.g.resident_jit_status(), p.g.jit_status())
    rng = np.random.default_rng(1400 + sched)
    every = list(range(K))

    def c(cells, seed, **kw):
        return _calls(rng, sc, sched, R, cells, seed, **kw)

    p.call(c(every, 1, epoch=1), 0.101)                                               # stores the images
    p.call(c(every, 1, epoch=1), 0.102)                                               # served from them
    p.call(c(every, 1, epoch=1), 0.102)                                               # now == last_update: no update
    p.call(c(every, 2, subset=True, pick=1), 0.103)                                   # user_id subsets, no cqi_epoch
    p.call(c([2, 0], 3, epoch=2), np.array([0.104, 0.1045]), cell_ids=[2, 0])         # a cell subset, a clock per cell
    p.call(c([1, 2, 0], 3, epoch=2), np.array([0.105, 0.1051, 0.1052]), cell_ids=[1, 2, 0])   # cell 1 stores, cells 2 and 0 reuse
    p.call(c(every, 4, epoch=3, subset=True, pick=2), 0.106)                          # named users under a number: stored ...
    p.call(c(every, 4, epoch=3, subset=True, pick=2), 0.107)                          # ... and reused with the same lists
    p.call(c([1], 5), 0.108, cell_ids=[1])                                            # one cell
    p.call(c(every, 6, epoch=4), 0.109)
    p.call(c([2, 1, 0], 6, epoch=4), 0.110, cell_ids=[2, 1, 0])                       # the same cells' images, permuted slots
    p.call(c(every, 7), 0.111)
    assert p.g.image_stats == p.ref.image_stats and all(x > 0 for x in p.g.image_stats), p.g.image_stats
    assert p.g.launch_count == p.n == 12 and p.ref.launch_count == 12   # the twin launch of a checked call is not counted
    code, msg = p.g.resident_jit_status()
    assert code == 1, (code, msg)
    # (scheduler 10 through this wrapper always asks for the upper_* lists, which the lean build does not write: the general build serves)
    served, other = ("general", "lean") if sched == 10 else ("lean", "general")
    if selfcheck == "2":
        assert f"{served} build: {VERIFIED}" in msg and f"{other} build: 0 checked call(s) agreed" in msg, msg
    else:
        assert "agreed" not in msg, msg
    assert p.g.jit_status()[0] == 0   # the plain pair was never asked for
    p.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the general build's paths
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sched,variant", [(9, "prb"), (9, "custom"), (7, "gates"), (10, "upper")])
def test_general_build_paths(rs, sched, variant, monkeypatch):
    """Per-PRB reports under a non-zero cqi_epoch (the cell's per-PRB store is written, then read), customised slices (algo_alpha = 1,
    hol_delay, prio_has_data), scheduler 7's required_rbs, scheduler 10's upper_* lists: the general build serves all of them."""
    monkeypatch.setenv("RS_JIT_SELFCHECK", "2")
    kw = dict(algo_alpha=[1, 1, 0, 1, 0], algo_beta=[0, 1, 0, 1, 0]) if variant == "custom" else {}
    sc = rs.SliceConfig(UES, weight=W, **kw)
    p = _Pair(rs, sc, R, K, sched, seed=70 + sched)
    rng = np.random.default_rng(1700 + sched + len(variant))
    every = list(range(K))
    for it in range(9):
        # a new number every third call: one stored call, two served from the image (and, for "prb", from the per-PRB store)
        p.call(_calls(rng, sc, sched, R, every, 20 + it // 3, epoch=1 + it // 3, pick=it // 3, variant=variant), 0.101 + 0.001 * it)
    p.call(_calls(rng, sc, sched, R, [2, 0], 30, subset=True, variant=variant), 0.111, cell_ids=[2, 0])
    assert p.g.image_stats == p.ref.image_stats and p.g.image_stats[0] > 0 and p.g.image_stats[1] > 0, p.g.image_stats
    code, msg = p.g.resident_jit_status()
    assert code == 1 and f"general build: {VERIFIED}" in msg and "lean build: 0 checked call(s) agreed" in msg, (code, msg)
    assert p.g.launch_count == 10
    p.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. against the oracle's DoSchedule loop at the sort shape
# ---------------------------------------------------------------------------------------------------------------------------

def test_against_the_oracle_at_the_sort_shape(rs, oracle, monkeypatch):
    """20 slices x 5 users, 64 RBGs of 8 (1 280 sort records on 512 threads), K = 2, 10 TTIs on the clock of the oracle's run loops:
    every rs_tti_out field of every TTI, the averages after TTIs 1, 2 and 10 bitwise; 8 of the 10 calls are checked ones."""
    monkeypatch.setenv("RS_JIT_SELFCHECK", "2")
    ues, n_rbgs, g_size, n_cells, n_ttis = [5] * 20, 64, 8, 2, 10
    w = [0.05] * 20
    sc = rs.SliceConfig(ues, weight=w)
    U = sc.n_users
    g = rs.GroupScheduler(sc, n_rbgs, g_size, n_cells, sched=9, jit_resident=True)
    cells = [oracle.Cell(ues, n_rbgs, g_size, 9, weights=w) for _ in range(n_cells)]
    ticks = oracle.clock_ticks(100, n_ttis)
    rands = [oracle.Rng(7300 + 17 * k) for k in range(n_cells)]
    rng = np.random.default_rng(7300)
    for k in range(n_cells):   # bearers created at 0.1 s, as in the reference's runs
        a0 = rng.uniform(1e3, 5e6, U)
        cells[k].set_avg_rate(a0)
        cells[k].set_last_update(0.1)
        g.set_avg(k, a0, 0.1)
    cqi = [None] * n_cells
    for it in range(n_ttis):
        calls, outs = [], []
        for k in range(n_cells):
            if it % 5 == 0:
                cqi[k] = synth_cqi(7300 + 1000 * k + it, (U, n_rbgs), HIST)
                cells[k].set_cqi(cqi[k])
            r0, r1 = rands[k].rand(), rands[k].rand()
            out = cells[k].new_out()
            assert cells[k].step(float(ticks[it]), r0, r1, out) == 0
            outs.append(out)
            calls.append(dict(cqi=cqi[k], rand0=r0, rand1=r1, cqi_epoch=1 + it // 5))
        res = g.schedule_tti_at(calls, ticks[it])
        assert g.kernel_name == JIT_NAME, g.resident_jit_status()
        for k in range(n_cells):
            _same(res[k], outs[k], f"TTI {it} cell {k}")
        if it + 1 in (1, 2, n_ttis):
            for k in range(n_cells):
                a, _, last = g.get_avg(k)
                assert a.tobytes() == cells[k].state()["avg_rate"].tobytes(), f"after TTI {it + 1}, cell {k}: averages"
                assert last == ticks[it]
    for k in range(n_cells):
        assert g.slice_offset(k).tobytes() == cells[k].state()["slice_state"].tobytes(), f"cell {k}: slice offsets"
    code, msg = g.resident_jit_status()
    assert code == 1 and f"lean build: {VERIFIED}" in msg, (code, msg)
    assert g.launch_count == n_ttis and g.image_stats == (8 * n_cells, 2 * n_cells, 0)
    g.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. more users than threads
# ---------------------------------------------------------------------------------------------------------------------------

def test_more_users_than_threads(rs, monkeypatch):
    """7 slices x 100 users, 25 RBGs of 4, one cell: the constant-stride update, gather and credit loops of the run-time build run more
    than once per thread (at most 512 threads); one of the 4 calls carries a user_id list of 300 users."""
    monkeypatch.setenv("RS_JIT_SELFCHECK", "2")
    ues, n_rbgs = [100] * 7, 25
    sc = rs.SliceConfig(ues, weight=[1.0 / 7] * 7)
    U = sc.n_users
    ref = rs.GroupScheduler(sc, n_rbgs, 4, 1, sched=9)
    g = rs.GroupScheduler(sc, n_rbgs, 4, 1, sched=9, jit_resident=True)
    rng = np.random.default_rng(44)
    a0 = rng.uniform(1e3, 5e6, U)
    for grp in (ref, g):
        grp.set_avg(0, a0, 0.1)
    for it in range(4):
        r0, r1 = _rand2(rng)
        kw = dict(cqi=synth_cqi(4400 + it, (U, n_rbgs), HIST), rand0=r0, rand1=r1, cqi_epoch=1 + it // 2)
        if it == 2:
            ids = np.sort(rng.choice(U, 300, replace=False)).astype(np.int32)
            kw.update(cqi=kw["cqi"][ids], user_id=ids, cqi_epoch=0)
        res, want = g.schedule_tti_at([kw], 0.101 + 0.001 * it)[0], ref.schedule_tti_at([kw], 0.101 + 0.001 * it)[0]
        _same(res, want, f"call {it}")
        assert g.kernel_name == JIT_NAME, g.resident_jit_status()
        if it == 0:   # the update of all 700 users, against the numpy expression
            assert g.get_avg(0)[0].tobytes() == _update(a0, np.zeros(U, np.int32), 0.1, 0.101).tobytes()
        assert _state(g, 1) == _state(ref, 1), f"call {it}: resident state"
        assert g.slice_offset(0).tobytes() == ref.slice_offset(0).tobytes()
        assert np.count_nonzero(g.get_avg(0)[1]) > 0
    code, msg = g.resident_jit_status()
    assert code == 1 and "lean build: 4 checked call(s) agreed" in msg, (code, msg)
    g.close()
    ref.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. names and independence
# ---------------------------------------------------------------------------------------------------------------------------

def test_names_and_independence_of_the_two_pairs(rs, monkeypatch):
    monkeypatch.setenv("RS_JIT_SELFCHECK", "2")
    sc = rs.SliceConfig(small.UES, weight=small.W)
    U = sc.n_users
    rng = np.random.default_rng(55)
    avg = rng.uniform(1e3, 5e6, U)

    def plain(p, seed):
        calls = [dict(c, avg_rate=avg) for c in _plain_calls(rng, K, U, seed)]
        before = _state(p.g, K)
        res, want = p.g.schedule_tti(calls), p.ref.schedule_tti(calls)
        for k in range(K):
            _same(res[k], want[k], f"plain call, cell {k}")
        assert _state(p.g, K) == before   # the resident state is neither read nor written
        p.same_state("after a plain call")

    # specialize_resident() only: plain calls stay on the built-in group kernel
    p = _Pair(rs, sc, small.R, K, 9, seed=5)
    assert p.g.kernel_name.startswith("rs_group_kernel<9,")   # nothing was called yet
    p.call(_calls(rng, sc, 9, small.R, range(K), 1), 0.101)
    plain(p, 500)
    assert p.g.kernel_name.startswith("rs_group_kernel<9,") and p.g.kernel_name == p.ref.kernel_name
    p.call(_calls(rng, sc, 9, small.R, range(K), 2), 0.102)
    assert p.g.jit_status()[0] == 0 and p.g.resident_jit_status()[0] == 1
    assert "lean build: 2 checked call(s) agreed" in p.g.resident_jit_status()[1]
    stats = rs.jit_cache_stats()
    p.g.specialize_resident()   # RS_OK, nothing built
    assert rs.jit_cache_stats() == stats
    p.close()
    # both: the name alternates, each status reports its own pair
    p = _Pair(rs, sc, small.R, K, 9, seed=6, both=True)
    assert p.g.jit_status()[0] == 1 and p.g.resident_jit_status()[0] == 1
    for it in range(3):
        plain(p, 600 + 10 * it)
        assert p.g.kernel_name == "rs_group_kernel_jit"
        p.call(_calls(rng, sc, 9, small.R, range(K), 10 + it), 0.101 + 0.001 * it)
        assert p.g.kernel_name == JIT_NAME
    assert "lean build: 3 checked call(s) agreed with the built-in kernel field by field, 5 to go" in p.g.jit_status()[1], p.g.jit_status()
    assert f"lean build: 3 checked call(s) agreed with {REF}, 5 to go" in p.g.resident_jit_status()[1], p.g.resident_jit_status()
    assert p.g.launch_count == 6
    p.close()
    # specialize() first, specialize_resident() later, between two calls
    g = rs.GroupScheduler(sc, small.R, G, K, sched=9, jit=True)
    for k in range(K):
        g.set_avg(k, avg, 0.1)
    g.schedule_tti_at(_calls(rng, sc, 9, small.R, range(K), 20), 0.101)
    assert g.kernel_name.startswith("rs_group_resident_kernel<9,") and g.resident_jit_status()[0] == 0
    before = _state(g, K)
    g.specialize_resident()
    assert _state(g, K) == before
    g.schedule_tti_at(_calls(rng, sc, 9, small.R, range(K), 21), 0.102)
    assert g.kernel_name == JIT_NAME
    g.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. a build that is wrong in its state alone
# ---------------------------------------------------------------------------------------------------------------------------

def test_a_wrong_resident_build_is_dropped_on_state_alone(rs, monkeypatch, tmp_path):
    """-DRS_FAULT_INJECT_RESIDENT: the run-time resident kernel credits every served user one byte more in the pending bytes (a wrong
    value, no address).  Its outputs are right; the first call's comparison of the resident stores drops the resident pair."""
    monkeypatch.delenv("RS_JIT_SELFCHECK", raising=False)
    monkeypatch.setenv("RS_JIT_EXTRA", "-DRS_FAULT_INJECT_RESIDENT")
    monkeypatch.setenv("RS_JIT_CACHE_DIR", str(tmp_path))
    sc = rs.SliceConfig(small.UES, weight=small.W)
    U = sc.n_users
    rng = np.random.default_rng(66)
    p = _Pair(rs, sc, small.R, K, 9, seed=6, both=True)
    assert p.g.resident_jit_status()[0] == 1 and p.g.jit_status()[0] == 1
    files = set(tmp_path.glob("*.rsco"))
    assert len(files) == 4
    resident_files = {f for f in files if b"-DRS_JIT_GROUP_RESIDENT=1" in f.read_bytes()}
    assert len(resident_files) == 2
    p.call(_calls(rng, sc, 9, small.R, range(K), 1), 0.101, served_by_jit=False)   # outputs and state: the built-in kernel's
    code, msg = p.g.resident_jit_status()
    assert code == -2 and "pending_bytes[" in msg and "cell " in msg and "checked call 1" in msg, (code, msg)
    assert "the built-in resident kernel serves" in msg, msg
    assert set(tmp_path.glob("*.rsco")) == files - resident_files, "the rejected resident builds are still in the cache"
    with pytest.raises(rs.RadioSaberError) as e:
        p.g.specialize_resident()
    assert e.value.code == -4 and "pending_bytes[" in str(e.value)   # RS_ERR_STATE, with the reason
    for it in range(1, 6):
        p.call(_calls(rng, sc, 9, small.R, range(K), 1 + it, subset=it % 2 == 1), 0.101 + 0.001 * it, served_by_jit=False)
    assert p.g.launch_count == 6
    # the plain pair built beside it is still in service
    calls = [dict(c, avg_rate=rng.uniform(1e3, 5e6, U)) for c in _plain_calls(rng, K, U, 700)]
    res, want = p.g.schedule_tti(calls), p.ref.schedule_tti(calls)
    for k in range(K):
        _same(res[k], want[k], f"plain call, cell {k}")
    assert p.g.jit_status()[0] == 1 and p.g.kernel_name == "rs_group_kernel_jit"
    p.close()
    # the same wrong build without the check really leaves wrong pending bytes (the injection bites)
    monkeypatch.setenv("RS_JIT_SELFCHECK", "0")
    monkeypatch.setenv("RS_JIT_EXTRA", "-DRS_FAULT_INJECT_RESIDENT -DRS_UNCHECKED_TWIN")  # (another key: the first one is rejected for this process)
    p = _Pair(rs, sc, small.R, K, 9, seed=6)
    calls = _calls(rng, sc, 9, small.R, range(K), 9)
    res, want = p.g.schedule_tti_at(calls, 0.101), p.ref.schedule_tti_at(calls, 0.101)
    assert p.g.kernel_name == JIT_NAME
    for k in range(K):
        _same(res[k], want[k], f"unchecked wrong build, cell {k}")   # the outputs are right ...
        mine, theirs = p.g.get_avg(k)[1], p.ref.get_avg(k)[1]
        served = theirs != 0
        assert served.any()
        np.testing.assert_array_equal(mine, theirs + served)          # ... the pending bytes are not
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
ues, R, G, K = [3, 4, 0, 2, 5], 12, 2, 3
U = sum(ues)
sc = rs.SliceConfig(ues, weight=[0.3, 0.2, 0.1, 0.15, 0.25])
g = rs.GroupScheduler(sc, R, G, K, sched=9)
g.specialize_resident()
ref = rs.GroupScheduler(sc, R, G, K, sched=9)
rng = np.random.default_rng(6)
for k in range(K):
    a0 = rng.uniform(1e3, 5e6, U)
    g.set_avg(k, a0, 0.1)
    ref.set_avg(k, a0, 0.1)
ok, names = True, set()
for it in range(16):   # 8 plain calls (the lean build), 8 with per-PRB reports (the general build)
    calls = []
    for k in range(K):
        cqi = synth_cqi(600 + 10 * it + k, (U, R), HIST)
        kw = dict(cqi=cqi, rand0=int(rng.integers(0, 2**31 - 1)), rand1=int(rng.integers(0, 2**31 - 1)))
        if it >= 8:
            kw = dict(kw, cqi=None, cqi_prb=np.repeat(cqi, G, axis=1))
        calls.append(kw)
    res, want = g.schedule_tti_at(calls, 0.101 + 0.001 * it), ref.schedule_tti_at(calls, 0.101 + 0.001 * it)
    names.add(g.kernel_name)
    for k in range(K):
        ok &= all(np.array_equal(getattr(res[k], f), getattr(want[k], f)) for f in FIELDS)
        ok &= all(np.array_equal(a, b) for a, b in zip(g.get_avg(k), ref.get_avg(k)))
        ok &= g.slice_offset(k).tobytes() == ref.slice_offset(k).tobytes()
out = dict(ok=bool(ok), status=g.resident_jit_status(), plain=g.jit_status()[0], kernels=sorted(names), launches=g.launch_count,
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
    first = _child(tmp_path)
    assert first["ok"] and first["status"][0] == 1 and first["kernels"] == [JIT_NAME] and first["launches"] == 16 and first["plain"] == 0, first
    assert f"general build: {VERIFIED}" in first["status"][1] and f"lean build: {VERIFIED}" in first["status"][1], first
    marks = sorted(f.read_bytes()[-8:].decode() for f in tmp_path.glob("*.rsco"))
    assert first["stats"]["misses"] == 2 and marks == ["VERIFIED", "VERIFIED"], (first, marks)
    second = _child(tmp_path)
    assert second["ok"] and second["stats"] == {"hits": 2, "misses": 0, "stores": 0, "rejected": 0}, second
    assert second["status"][0] == 1 and second["kernels"] == [JIT_NAME] and second["launches"] == 16, second
    assert "general build: carries the self-check mark" in second["status"][1] and "lean build: carries the self-check mark" in second["status"][1], second
    assert "agreed" not in second["status"][1], second   # no call was a checked one
