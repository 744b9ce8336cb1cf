"""rs_group_specialize: a group's own run-time builds of the one-TTI kernel (general and lean), checked against the built-in group kernel
during their first calls.  Against K independent built-in contexts for every scheduler, against the CPU oracle at the sort shape with
mixed image modes and subset calls, specialising mid-life, more slots than compute units, a deliberately wrong build, and the
self-check mark that travels to the next process through the cache file."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import synth_cqi
from test_gpu_group import HIST, SCHEDS, _ewma, _same, _twin_calls

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
SMALL = ([3, 4, 0, 2, 5], 12, 2)          # ragged slices, an empty slice; _twin_calls deals per-cell user subsets
SMALL_W = [0.3, 0.2, 0.1, 0.15, 0.25]
SORT = ([5] * 20, 64, 8)                  # 1 280 sort records on 512 threads: three position slots, the last held by waves 0-3 only
VERIFIED = "verified (8 checked calls agreed with the built-in kernel field by field)"


def _rand2(rng):
    return int(rng.integers(0, 2**31 - 1)), int(rng.integers(0, 2**31 - 1))


# ---------------------------------------------------------------------------------------------------------------------------
# 1. equals independent contexts, every scheduler, both builds
# ---------------------------------------------------------------------------------------------------------------------------

CASES = ([(s, v) for s in SCHEDS for v in ("plain", "prb")] + [(1, "gates"), (7, "gates"), (9, "custom")])


@pytest.mark.parametrize("sched,variant", CASES)
def test_specialised_group_equals_independent_contexts(rs, sched, variant, monkeypatch):
    """12 TTIs with RS_JIT_SELFCHECK=2: 8 checked calls and 4 unchecked ones of the build the variant selects ("plain": the lean build,
    everything else -- and every call of scheduler 10, whose upper_* lists are asked for -- the general one).  Every field and the slice state equal K built-in TtiScheduler twins bit for bit."""
    monkeypatch.setenv("RS_JIT_SELFCHECK", "2")
    ues, R, G = SMALL
    K, n_ttis = 5, 12
    kw = dict(algo_alpha=[1, 1, 0, 1, 0], algo_beta=[0, 1, 0, 1, 0]) if variant == "custom" else {}
    sc = rs.SliceConfig(ues, weight=SMALL_W, **kw)
    g = rs.GroupScheduler(sc, R, G, K, sched=sched, jit=True)
    assert g.kernel_name == "rs_group_kernel_jit", g.jit_status()
    twins = [rs.TtiScheduler(sc, R, G, sched=sched) for _ in range(K)]
    rng = np.random.default_rng(900 + 7 * sched + len(variant))
    for it in range(n_ttis):
        calls = _twin_calls(rng, sc, sched, R, G, K, it, variant, seed=80000 + sched)
        res = g.schedule_tti(calls)
        for k in range(K):
            one = twins[k].schedule_tti(**calls[k])
            _same(res[k], one, f"sched {sched} {variant} TTI {it} cell {k}", upper=sched == 10)
            assert g.slice_offset(k).tobytes() == twins[k].slice_offset.tobytes(), f"sched {sched} {variant} TTI {it} cell {k}: slice state"
    code, msg = g.jit_status()
    # (scheduler 10 through this wrapper always asks for the upper_* lists, which the lean build does not write: the general build serves)
    served, other = ("lean", "general") if variant == "plain" and sched != 10 else ("general", "lean")
    assert code == 1 and f"{served} build: {VERIFIED}" in msg, (code, msg)
    assert f"{other} build: 0 checked call(s) agreed" in msg, msg  # never picked: still to be checked
    assert g.kernel_name == "rs_group_kernel_jit"
    assert g.launch_count == n_ttis  # the twin launch of a checked call is not counted
    g.close()
    for t in twins:
        t.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. against the oracle at the sort shape: mixed image modes, subset calls
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sched", [9, 10])
def test_specialised_group_against_the_oracle_at_the_sort_shape(rs, oracle, sched, monkeypatch):
    """K = 7, 30 TTIs.  Cell k's reports and number change every 10 TTIs, k TTIs out of step with cell 0's, so one launch mixes slots
    that store an image with slots served from one (those send a poisoned block); the last cell always passes 0.  Every third call
    names a permuted subset of the cells."""
    monkeypatch.setenv("RS_JIT_SELFCHECK", "2")
    ues, R, G = SORT
    K, n_ttis, S, U = 7, 30, len(ues), sum(ues)
    sc = rs.SliceConfig(ues, weight=[1.0 / S] * S)
    g = rs.GroupScheduler(sc, R, G, K, sched=sched, jit=True)
    assert g.kernel_name == "rs_group_kernel_jit", g.jit_status()
    cells = [oracle.Cell(ues, R, G, sched, weights=[1.0 / S] * S) for _ in range(K)]
    rng = np.random.default_rng(1200 + sched)
    avg = [rng.uniform(1e3, 5e6, U) for _ in range(K)]
    cqi, period, held = [None] * K, [-1] * K, [None] * K
    poisoned = np.full((U, R), 15, np.uint8)
    want = [0, 0, 0]
    mixed = 0
    for it in range(n_ttis):
        named = list(range(K))
        if it % 3 == 2:
            named = [int(x) for x in rng.permutation(K)[: 2 + it % 4]]
        calls, outs, modes = [], [], set()
        for k in named:
            if (it + k) // 10 != period[k]:
                period[k] = (it + k) // 10
                cqi[k] = synth_cqi(29000 + 1000 * sched + 100 * k + period[k], (U, R), HIST)
            number = 0 if k == K - 1 else 1 + period[k]
            mode = 0 if number == 0 else (2 if held[k] == number else 1)
            held[k] = number if number else None
            want[{2: 0, 1: 1, 0: 2}[mode]] += 1
            modes.add(mode)
            r0, r1 = _rand2(rng)
            cells[k].set_cqi(cqi[k])
            out = cells[k].new_out()
            assert cells[k].allocate(avg[k], r0, r1, out) == 0
            outs.append(out)
            calls.append(dict(cqi=poisoned if mode == 2 else cqi[k], avg_rate=avg[k].copy(), rand0=r0, rand1=r1, cqi_epoch=number))
        mixed += {1, 2} <= modes
        res = g.schedule_tti(calls, cell_ids=named)
        for j, k in enumerate(named):
            _same(res[j], outs[j], f"sched {sched} TTI {it} cell {k} (slot {j})", upper=sched == 10)
            avg[k] = _ewma(avg[k], res[j].user_tbs_bits)
    assert mixed >= 3, "no launch mixed stored and reused images"
    assert g.image_stats == tuple(want) and want[0] > want[1] > 0 and want[2] > 0
    assert g.launch_count == n_ttis
    code, msg = g.jit_status()
    assert code == 1 and f"{'lean' if sched == 9 else 'general'} build: {VERIFIED}" in msg, (code, msg)  # (10: the upper_* lists)
    for k in range(K):
        assert g.slice_offset(k).tobytes() == cells[k].state()["slice_state"].tobytes(), f"cell {k}: slice offsets"
    g.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. specialising mid-life
# ---------------------------------------------------------------------------------------------------------------------------

def test_specialising_between_two_calls_keeps_state_and_images(rs):
    ues, R, G = SMALL
    K, U = 5, sum(ues)
    sc = rs.SliceConfig(ues, weight=SMALL_W)
    g = rs.GroupScheduler(sc, R, G, K, sched=9)
    twins = [rs.TtiScheduler(sc, R, G, sched=9) for _ in range(K)]
    rng = np.random.default_rng(31)
    truth = [synth_cqi(310 + k, (U, R), HIST) for k in range(K)]
    poisoned = np.full((U, R), 15, np.uint8)

    def step(it):
        calls = []
        for k in range(K):
            r0, r1 = _rand2(rng)
            calls.append(dict(cqi=truth[k], avg_rate=rng.uniform(1.0, 1e6, U), rand0=r0, rand1=r1, cqi_epoch=7))
        # after the first call every cell is served from its image: the block that travels is not the truth
        res = g.schedule_tti(calls if it == 0 else [dict(c, cqi=poisoned) for c in calls])
        for k in range(K):
            _same(res[k], twins[k].schedule_tti(**calls[k]), f"TTI {it} cell {k}")
            assert g.slice_offset(k).tobytes() == twins[k].slice_offset.tobytes(), f"TTI {it} cell {k}: slice state"

    for it in range(5):
        step(it)
    assert g.kernel_name.startswith("rs_group_kernel<9,") and g.jit_status()[0] == 0
    assert g.image_stats == (4 * K, K, 0)
    g.specialize()
    assert g.kernel_name == "rs_group_kernel_jit" and g.jit_status()[0] == 1
    step(5)
    assert g.image_stats == (5 * K, K, 0), "the first call after specialize() was not served from the built-in kernel's images"
    stats = rs.jit_cache_stats()
    g.specialize()  # RS_OK, nothing built
    assert rs.jit_cache_stats() == stats and g.jit_status()[0] == 1
    for it in range(6, 15):
        step(it)
    assert g.image_stats == (14 * K, K, 0) and g.launch_count == 15
    g.close()
    for t in twins:
        t.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. more slots than compute units
# ---------------------------------------------------------------------------------------------------------------------------

def test_three_hundred_slots_on_the_run_time_entry_point(rs, monkeypatch):
    """K = 300: the workgroups are not all resident at once, so the completion counter of rs_group_kernel_jit works across dispatch
    rounds.  RS_JIT_SELFCHECK=0: every call completes by the run-time build's own polled word.  Against a built-in group of the same K."""
    monkeypatch.setenv("RS_JIT_SELFCHECK", "0")
    ues, R, G = SMALL
    K = 300
    sc = rs.SliceConfig(ues, weight=SMALL_W)
    g = rs.GroupScheduler(sc, R, G, K, sched=8, jit=True)
    ref = rs.GroupScheduler(sc, R, G, K, sched=8)
    assert g.kernel_name == "rs_group_kernel_jit" and ref.kernel_name.startswith("rs_group_kernel<8,")
    rng = np.random.default_rng(300)
    for it in range(3):
        calls = _twin_calls(rng, sc, 8, R, G, K, it, "plain", seed=3300)
        res, want = g.schedule_tti(calls), ref.schedule_tti(calls)
        for k in range(K):
            _same(res[k], want[k], f"TTI {it} cell {k}")
    for k in range(K):
        assert g.slice_offset(k).tobytes() == ref.slice_offset(k).tobytes(), f"cell {k}: slice state"
    assert g.launch_count == 3
    assert g.jit_status()[0] == 1 and "agreed" not in g.jit_status()[1], g.jit_status()  # no call was a checked one
    g.close()
    ref.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. a wrong build is dropped on its first call
# ---------------------------------------------------------------------------------------------------------------------------

def _drive_oracle(rs, oracle, g, sched, ues, R, G, K, n_calls, seed):
    S, U = len(ues), sum(ues)
    cells = [oracle.Cell(ues, R, G, sched, weights=[1.0 / S] * S) for _ in range(K)]
    rng = np.random.default_rng(seed)
    avg = [rng.uniform(1e3, 5e6, U) for _ in range(K)]
    cqi = [synth_cqi(seed * 100 + k, (U, R), HIST) for k in range(K)]
    for it in range(n_calls):
        calls, outs = [], []
        for k in range(K):
            r0, r1 = _rand2(rng)
            cells[k].set_cqi(cqi[k])
            out = cells[k].new_out()
            assert cells[k].allocate(avg[k], r0, r1, out) == 0
            outs.append(out)
            calls.append(dict(cqi=cqi[k], avg_rate=avg[k].copy(), rand0=r0, rand1=r1, cqi_epoch=1))
        res = g.schedule_tti(calls)
        for k in range(K):
            _same(res[k], outs[k], f"call {it} cell {k}")
            avg[k] = _ewma(avg[k], outs[k].user_tbs_bits)
        if it == 0:
            yield
    for k in range(K):
        assert g.slice_offset(k).tobytes() == cells[k].state()["slice_state"].tobytes(), f"cell {k}: slice offsets"
    yield


def test_a_wrong_group_build_is_dropped_on_its_first_call(rs, oracle, monkeypatch, tmp_path):
    """-DRS_FAULT_INJECT_DIRECT: the run-time one-TTI kernel reports a byte more in every transport block (wrong values only).  The first
    call runs beside the built-in group kernel, differs and is served by it: all 10 calls return the oracle's numbers."""
    monkeypatch.delenv("RS_JIT_SELFCHECK", raising=False)
    monkeypatch.setenv("RS_JIT_EXTRA", "-DRS_FAULT_INJECT_DIRECT")
    monkeypatch.setenv("RS_JIT_CACHE_DIR", str(tmp_path))
    ues, R, G, K = [5] * 20, 25, 4, 4
    sc = rs.SliceConfig(ues)
    g = rs.GroupScheduler(sc, R, G, K, sched=9, jit=True)
    assert g.jit_status()[0] == 1 and g.kernel_name == "rs_group_kernel_jit"
    assert len(list(tmp_path.glob("*.rsco"))) == 2
    drive = _drive_oracle(rs, oracle, g, 9, ues, R, G, K, 10, seed=5)
    next(drive)  # call 1
    code, msg = g.jit_status()
    assert code == -2 and "cell " in msg and "user_tbs_bits" in msg and "checked call 1" in msg and "built-in kernels serve" in msg, (code, msg)
    assert g.kernel_name.startswith("rs_group_kernel<9,")
    assert not list(tmp_path.glob("*.rsco")), "the rejected builds are still in the cache"
    with pytest.raises(rs.RadioSaberError) as e:
        g.specialize()
    assert e.value.code == -4 and "user_tbs_bits" in str(e.value)  # RS_ERR_STATE, with the reason
    next(drive)  # calls 2-10 and the final slice offsets
    assert g.launch_count == 10
    g.close()
    # the same wrong build without the check really returns wrong numbers (the injection bites)
    monkeypatch.setenv("RS_JIT_SELFCHECK", "0")
    monkeypatch.setenv("RS_JIT_EXTRA", "-DRS_FAULT_INJECT_DIRECT -DRS_UNCHECKED_TWIN")  # (another key: the first one is rejected for this process)
    g = rs.GroupScheduler(sc, R, G, K, sched=9, jit=True)
    with pytest.raises(AssertionError):
        next(_drive_oracle(rs, oracle, g, 9, ues, R, G, K, 2, seed=5))
    g.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the mark travels
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
ues, R, G, K = [3, 4, 0, 2, 5], 12, 2, 5
U = sum(ues)
sc = rs.SliceConfig(ues, weight=[0.3, 0.2, 0.1, 0.15, 0.25])
g = rs.GroupScheduler(sc, R, G, K, sched=9)
g.specialize()
twins = [rs.TtiScheduler(sc, R, G, sched=9) for _ in range(K)]
rng = np.random.default_rng(6)
ok = True
for it in range(12):
    calls = [dict(cqi=synth_cqi(600 + 10 * it + k, (U, R), HIST), avg_rate=rng.uniform(1.0, 1e6, U), rand0=int(rng.integers(0, 2**31 - 1)),
                  rand1=int(rng.integers(0, 2**31 - 1))) for k in range(K)]
    res = g.schedule_tti(calls)
    for k in range(K):
        one = twins[k].schedule_tti(**calls[k])
        ok &= all(np.array_equal(getattr(res[k], f), getattr(one, f)) for f in FIELDS)
        ok &= g.slice_offset(k).tobytes() == twins[k].slice_offset.tobytes()
out = dict(ok=bool(ok), status=g.jit_status(), kernel=g.kernel_name, launches=g.launch_count, stats=rs.jit_cache_stats())
g.close()
for t in twins:
    t.close()
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
    # 12 plain calls: the lean build served them all and passed its 8; the general build, never picked, stays unchecked
    assert first["ok"] and first["status"][0] == 1 and first["kernel"] == "rs_group_kernel_jit" and first["launches"] == 12, first
    assert f"lean build: {VERIFIED}" in first["status"][1], first
    assert "general build: 0 checked call(s) agreed" in first["status"][1] and "8 to go" in first["status"][1], first
    marks = sorted(f.read_bytes()[-8:].decode() for f in tmp_path.glob("*.rsco"))
    assert first["stats"]["misses"] == 2 and marks == ["UNCHECKD", "VERIFIED"], (first, marks)
    second = _child(tmp_path)
    assert second["ok"] and second["stats"] == {"hits": 2, "misses": 0, "stores": 0, "rejected": 0}, second
    assert second["status"][0] == 1 and "lean build: carries the self-check mark" in second["status"][1], second
