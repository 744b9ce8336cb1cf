"""GPU: grant records of unlogged launches of backlogged batches (rs_batch_run_grant_records) -- one 32-byte record per (TTI, user)
that DoStopSchedule credits, exact against the CPU oracle.

Expected records come from the oracle's run_synth log: user, tbs_bits, bytes = min(tbs_bits // 8, 1e8) and, for the schedulers other
than 10, rbg_mask from rbg_to_user.  The oracle's log has no per-user PRB count, final CQI or MCS: nprb, final_cqi and mcs are compared
with the uinfo rows of a twin batch's run_logged on the built-in kernels -- DEVICE == DEVICE for these three fields (the logged rows
themselves are oracle-checked by tests/test_gpu_parity.py and tests/test_gpu_dropin_oracle.py).  Scheduler 10's map is a convention
of this build (the lowest slice's user per RBG), so its rbg_mask is tested by properties against the twin's map.  Every record of
every case is compared, and the final state after run_grant_records equals the oracle's, as in test_gpu_parity._check_batch.

Inputs: the suite's CQI histogram; cell 0 has synth_cqi(1, ...) and rand() seed 805290992, cell 1 another grid and seed."""
import functools
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import GOLDEN, synth_cqi
from radiosaber_amd import logfmt

ROOT = Path(__file__).resolve().parents[1]
HIST = (152600, 56656, 270880, 2088792, 3509504, 1595568, 4145392, 5295816, 1903424,
        6890232, 4770864, 2842552, 3579624, 96000, 1227696)
RS_ERR_INVALID, RS_ERR_HIP, RS_ERR_STATE, RS_ERR_RANGE = -1, -3, -4, -5
N_CELLS = 2
SEEDS = np.array([805290992, 805290992 + 7919], np.uint32)

# name: (scheduler, users per slice, RBGs, PRBs per RBG, TTIs)
INPUTS = {
    "9-543-8x2": (9, [5, 4, 3], 8, 2, 45),
    "9-222-25x4": (9, [2, 2, 2], 25, 4, 45),
    "9-20x5-25x4": (9, [5] * 20, 25, 4, 45),
    "9-20x5-64x8": (9, [5] * 20, 64, 8, 45),
    "9-444-64x8": (9, [4, 4, 4], 64, 8, 45),
    "8-20x5-25x4": (8, [5] * 20, 25, 4, 45),
    "101-20x5-25x4": (101, [5] * 20, 25, 4, 45),
    "103-20x5-25x4": (103, [5] * 20, 25, 4, 45),
    "7-20x5-25x4": (7, [5] * 20, 25, 4, 45),
    "1-20x5-25x4": (1, [5] * 20, 25, 4, 45),
    "1-20x50-25x4": (1, [50] * 20, 25, 4, 8),     # the one-wave-per-RBG scan
    "10-20x5-25x4": (10, [5] * 20, 25, 4, 45),    # more grants than RBGs
    "10-ragged-25x4": (10, [3, 7, 0, 1, 12], 25, 4, 45),   # RBGs left empty
}


def _grids(ues, R, n_ttis, refresh=40, n_epochs=None):
    n_epochs = n_epochs or (n_ttis + refresh - 1) // refresh
    return np.stack([synth_cqi(1 + c, (n_epochs, sum(ues), R), HIST) for c in range(N_CELLS)])


@functools.lru_cache(maxsize=None)
def _oracle_run(name, phy=0, refresh=40, n_epochs=None):
    """-> per cell (log, final state) of the oracle, computed once and shared (nothing writes to it)"""
    from oracle import oracle_py
    sched, ues, R, G, n_ttis = INPUTS[name]
    grids = _grids(ues, R, n_ttis, refresh, n_epochs)
    out = []
    for c in range(N_CELLS):
        cell = oracle_py.Cell(ues, R, G, sched)
        g = grids[c]
        if n_epochs:   # (cycling epochs: the oracle gets the grids tiled)
            g = np.tile(g, ((n_ttis + refresh * n_epochs - 1) // (refresh * n_epochs), 1, 1))
        logs = cell.run_synth(g, int(SEEDS[c]), n_ttis, refresh=refresh, phy_error_draws=phy)
        out.append((logs, cell.state()))
    return out


def _batch(rs, name, phy=0, refresh=40, n_epochs=None, **kw):
    sched, ues, R, G, n_ttis = INPUTS[name]
    b = rs.BatchScheduler(rs.SliceConfig(ues), R, G, N_CELLS, sched=sched, phy_error_draws=bool(phy), cqi_refresh=refresh,
                          cqi_epoch_wrap=bool(n_epochs), **kw)
    b.seed(SEEDS)
    b.upload_cqi_epochs(_grids(ues, R, n_ttis, refresh, n_epochs))
    return b


_TWINS = {}


def _twin_rows(rs, name, phy=0, refresh=40, n_epochs=None):
    """uinfo's three fields and the map of a logged twin on the built-in kernels, once per input (device == device, see above)"""
    key = (name, phy, refresh, n_epochs)
    if key not in _TWINS:
        b = _batch(rs, name, phy, refresh, n_epochs, jit=False)
        got = b.run_logged(INPUTS[name][4])
        b.close()
        _TWINS[key] = {k: got[k] for k in ("nprb", "final_cqi", "mcs", "rbg_to_user", "tbs_bits")}
    return _TWINS[key]


def _expected(rs, name, c, t0=0, t1=None, **how):
    """cell c's records of TTIs t0 .. t1 - 1: the oracle's, with the twin's nprb / final_cqi / mcs (and no mask for scheduler 10)"""
    sched, ues, R, G, n_ttis = INPUTS[name]
    logs, _ = _oracle_run(name, **how)[c]
    tw = _twin_rows(rs, name, **how)
    t1 = n_ttis if t1 is None else t1
    uinfo = tw["nprb"][c] | (tw["final_cqi"][c] << 16) | (tw["mcs"][c] << 24)
    recs = logfmt.grant_records_from_rows(logs["tbs_bits"][t0:t1], uinfo[t0:t1], None if sched == 10 else logs["rbg_to_user"][t0:t1], first_tti=t0)
    assert (recs["nprb"] > 0).all() and (recs["final_cqi"] >= 1).all() and (recs["final_cqi"] <= 15).all()
    return recs


def _same(got, want, what, sched):
    assert got.dtype == want.dtype and len(got) == len(want), f"{what}: {len(got)} records against {len(want)}"
    if sched == 10:   # (the mask: by properties, _upper_masks)
        got, want = got.copy(), want.copy()
        got["rbg_mask"] = want["rbg_mask"] = 0
    bad = np.flatnonzero(got != want)[:3]
    assert got.tobytes() == want.tobytes(), f"{what}: first differences {[(got[i], want[i]) for i in bad]}"


def _upper_masks(rs, name, c, recs, t0=0, **how):
    """scheduler 10: popcount * G == nprb; the union over a TTI's records == the RBGs the map gives away; the map's user has its bit"""
    _, _, R, G, n_ttis = INPUTS[name]
    m = _twin_rows(rs, name, **how)["rbg_to_user"][c]
    pop = np.array([bin(int(x)).count("1") for x in recs["rbg_mask"]])
    assert (pop * G == recs["nprb"]).all() and (recs["rbg_mask"] >> np.uint64(R) == 0).all()
    for n in np.unique(recs["tti"]):
        mine = recs[recs["tti"] == n]
        union = int(np.bitwise_or.reduce(mine["rbg_mask"]))
        assert union == sum(1 << r for r in range(R) if m[n, r] >= 0), f"cell {c}, TTI {n}: the masks' union against the map"
        for r in np.flatnonzero(m[n] >= 0):
            (owner,) = mine[mine["user"] == m[n, r]]
            assert int(owner["rbg_mask"]) >> int(r) & 1, f"cell {c}, TTI {n}, RBG {r}"


def _check_lists(rs, name, got, what, t0=0, t1=None, **how):
    sched = INPUTS[name][0]
    assert len(got) == N_CELLS
    for c in range(N_CELLS):
        _same(got[c], _expected(rs, name, c, t0, t1, **how), f"{what}, cell {c}", sched)
        if sched == 10:
            _upper_masks(rs, name, c, got[c], **how)


def _check_final(b, name, what, **how):
    st = b.state()
    for c in range(N_CELLS):
        ost = _oracle_run(name, **how)[c][1]
        np.testing.assert_array_equal(st["cum_bytes"][c], ost["cum_bytes"], err_msg=f"{what} cell {c} cum_bytes")
        np.testing.assert_array_equal(st["cum_rbs"][c], ost["cum_rbs"], err_msg=f"{what} cell {c} cum_rbs")
        assert st["avg_rate"][c].tobytes() == ost["avg_rate"].tobytes(), f"{what} cell {c}: PF averages differ"
        assert st["slice_state"][c].tobytes() == ost["slice_state"].tobytes(), f"{what} cell {c}: slice state differs"


def _builtin_name(b):
    return b.kernel_name.startswith("rs_cell_kernel<")


# ---------------------------------------------------------------- the inputs are what the issue says they are (no GPU)

def test_the_inputs(oracle):
    """Every TTI of every non-UpperBound input uses RBG R - 1 (the masks' top bit, bit 63 at 64 RBGs); a TTI has several grants, above
    the number of RBGs for UpperBound with 20 slices; the ragged UpperBound input leaves RBGs empty."""
    for name, (sched, ues, R, G, n_ttis) in INPUTS.items():
        logs = _oracle_run(name)[0][0]
        grants = (logs["tbs_bits"] // 8 > 0).sum(1)
        assert grants.min() >= 2, (name, grants.min())
        if sched != 10:
            assert (logs["rbg_to_user"][:, R - 1] >= 0).all(), name
            assert grants.max() <= min(sum(ues), R)
    assert (_oracle_run("10-20x5-25x4")[0][0]["tbs_bits"] // 8 > 0).sum(1).max() > 25
    assert (_oracle_run("9-20x5-64x8")[0][0]["tbs_bits"] // 8 > 0).sum(1).max() > 32
    held = np.bincount(_oracle_run("7-20x5-25x4")[0][0]["rbg_to_user"][0], minlength=100).max()
    assert held >= 5   # (NVS: the served slice's users hold many RBGs each)


# ---------------------------------------------------------------- GPU

@pytest.mark.gpu
@pytest.mark.parametrize("name", list(INPUTS))
def test_records_on_the_built_in_kernels(rs, oracle, name):
    sched, ues, R, G, n_ttis = INPUTS[name]
    b = _batch(rs, name, jit=False)
    want_bound = min(sum(ues), R) if sched != 10 else sum(min(n, R) for n in ues)
    assert b.grant_bound() == want_bound
    got = b.run_grant_records(n_ttis)
    assert _builtin_name(b)
    _check_lists(rs, name, got, f"{name}, built-in")
    for c in range(N_CELLS):
        assert np.bincount(got[c]["tti"], minlength=n_ttis).max() <= want_bound
    _check_final(b, name, f"{name}, built-in")
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lean", [False, True])
@pytest.mark.parametrize("name", list(INPUTS))
def test_records_on_the_run_time_builds(rs, oracle, name, lean, monkeypatch):
    """general: one launch of all TTIs; lean: RS_JIT_LEAN_MIN_TTIS=1.  Each variant passes its self-check with records on first."""
    if lean:
        monkeypatch.setenv("RS_JIT_LEAN_MIN_TTIS", "1")
    n_ttis = INPUTS[name][4]
    b = _batch(rs, name, jit=True)
    got = b.run_grant_records(n_ttis)
    assert b.kernel_name == ("rs_cell_kernel_jit[lean,records]" if lean else "rs_cell_kernel_jit[records]"), (b.kernel_name, b.jit_status())
    st = b.jit_status()
    assert st[0] == 1 and ("agree, state and records" in st[1] or "carries the self-check mark" in st[1]), st
    _check_lists(rs, name, got, f"{name}, {'lean' if lean else 'general'} records variant")
    _check_final(b, name, f"{name}, {'lean' if lean else 'general'} records variant")
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lean", [False, True])
def test_records_of_a_streamed_batch(rs, oracle, lean, monkeypatch):
    """cqi_refresh = 2 with cycling epochs, scheduler 8: the streamed build's records variant (the next grid is fetched beside P5)"""
    if lean:
        monkeypatch.setenv("RS_JIT_LEAN_MIN_TTIS", "1")
    name, how = "8-20x5-25x4", dict(refresh=2, n_epochs=5)
    b = _batch(rs, name, jit=True, **how)
    got = b.run_grant_records(45)
    assert b.kernel_name == ("rs_cell_kernel_jit[lean,streamed,records]" if lean else "rs_cell_kernel_jit[streamed,records]"), b.jit_status()
    _check_lists(rs, name, got, "streamed", **how)
    _check_final(b, name, "streamed", **how)
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,jit", [("9-543-8x2", True), ("9-222-25x4", False), ("1-20x5-25x4", True)])
def test_records_with_64_threads(rs, oracle, name, jit):
    """wave 0 is the only wave: it scans, sorts, allocates and writes the records"""
    b = _batch(rs, name, jit=jit, threads_per_cell=64)
    got = b.run_grant_records(45)
    assert b.kernel_name == "rs_cell_kernel_jit[records]" if jit else _builtin_name(b), b.kernel_name
    _check_lists(rs, name, got, f"{name}, 64 threads")
    _check_final(b, name, f"{name}, 64 threads")
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,jit", [("9-20x5-25x4", True), ("8-20x5-25x4", False), ("7-20x5-25x4", True)])
def test_records_with_the_error_models_draws(rs, oracle, name, jit):
    b = _batch(rs, name, phy=1, jit=jit)
    got = b.run_grant_records(45)
    _check_lists(rs, name, got, f"{name}, phy_error_draws", phy=1)
    _check_final(b, name, f"{name}, phy_error_draws", phy=1)
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("jit", [False, True])
@pytest.mark.parametrize("name", ["9-20x5-25x4", "7-20x5-25x4", "1-20x5-25x4", "10-20x5-25x4"])
def test_two_launches_concatenate(rs, oracle, name, jit):
    """7 + 38 TTIs: tti goes on counting across launches, the concatenation is one launch's list; a plain run in between moves it on too"""
    b = _batch(rs, name, jit=jit)
    first = b.run_grant_records(7)
    _check_lists(rs, name, first, f"{name}, TTIs 0 .. 6", 0, 7)
    second = b.run_grant_records(38)
    _check_lists(rs, name, second, f"{name}, TTIs 7 .. 44", 7, 45)
    sched = INPUTS[name][0]
    for c in range(N_CELLS):
        _same(np.concatenate([first[c], second[c]]), _expected(rs, name, c), f"{name}, both launches, cell {c}", sched)
    _check_final(b, name, f"{name}, two launches")
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("jit", [False, True])
@pytest.mark.parametrize("name", ["9-20x5-25x4", "10-20x5-25x4"])
def test_capacity_and_overflow(rs, oracle, name, jit):
    """cap exactly the largest count: complete.  cap = that - 3: RS_ERR_RANGE, n_recs is the count as counted, nothing is written at or
    behind the capacity; the records of all TTIs before the one that overflowed are exact (nothing is asserted about the split TTI), the
    final state is the oracle's, and the next call is exact."""
    sched, _, _, _, n_ttis = INPUTS[name]
    n = 30
    want = [_expected(rs, name, c, 0, n) for c in range(N_CELLS)]
    count = max(len(w) for w in want)
    b = _batch(rs, name, jit=jit)
    got = b.run_grant_records(n, cap=count)
    _check_lists(rs, name, got, f"{name}, cap == count", 0, n)
    b.close()
    b = _batch(rs, name, jit=jit)
    cap = min(len(w) for w in want) - 3
    with pytest.raises(rs.RadioSaberError) as e:
        b.run_grant_records(n, cap=cap)
    assert e.value.code == RS_ERR_RANGE and "cell 0 " in str(e.value), str(e.value)
    assert e.value.counts.tolist() == [len(w) for w in want]
    for c in range(N_CELLS):
        part = e.value.records[c]
        assert len(part) == cap
        split = int(want[c]["tti"][cap])           # the TTI whose records did not all fit
        whole = part[part["tti"] < split]
        _same(whole, want[c][want[c]["tti"] < split], f"{name}, cell {c}: the TTIs before the overflow", sched)
        assert (part["tti"] <= split).all()
    nxt = b.run_grant_records(n_ttis - n)
    _check_lists(rs, name, nxt, f"{name}, the call after the overflow", n, n_ttis)
    _check_final(b, name, f"{name}, after an overflow")
    b.close()


@pytest.mark.gpu
def test_refusals_launch_nothing(rs, oracle, monkeypatch):
    """Each refusal is checked before anything is launched: the batch does not move, the caller's arrays are not written, and the next
    call succeeds."""
    name = "9-222-25x4"
    L = rs.lib()
    b = _batch(rs, name, jit=False)
    first = b.run_grant_records(2)
    recs = np.zeros((N_CELLS, 64), rs.api.BATCH_GRANT_RECORD)
    n = np.full(N_CELLS, -7, np.int64)
    pn = n.ctypes.data_as(L.rs_batch_run_grant_records.argtypes[4])
    before = (b.clock(), b.state(), b.checkpoint())
    for args, code, word in (((1, 64, None, pn), RS_ERR_INVALID, "null"), ((1, 64, recs.ctypes.data, None), RS_ERR_INVALID, "null"),
                             ((1, 0, recs.ctypes.data, pn), RS_ERR_INVALID, "cap"), ((0, 64, recs.ctypes.data, pn), RS_ERR_INVALID, "n_ttis"),
                             ((32769, 64, recs.ctypes.data, pn), RS_ERR_INVALID, "32768")):
        assert L.rs_batch_run_grant_records(b._h, *args) == code, args
        assert word in L.rs_last_error().decode(), (args, L.rs_last_error().decode())
    # the device block that cannot be had: RS_RECORDS_MAX_BYTES, by the path of a failed allocation
    monkeypatch.setenv("RS_RECORDS_MAX_BYTES", "1")
    assert L.rs_batch_run_grant_records(b._h, 4, 64, recs.ctypes.data, pn) == RS_ERR_HIP and "no device block of" in L.rs_last_error().decode()
    monkeypatch.delenv("RS_RECORDS_MAX_BYTES")
    after = (b.clock(), b.state(), b.checkpoint())
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before[0], after[0]))
    assert all(before[1][k].tobytes() == after[1][k].tobytes() for k in before[1]) and before[2] == after[2]
    assert not recs.view(np.uint8).any() and (n == -7).all()
    rest = b.run_grant_records(43)
    for c in range(N_CELLS):
        _same(np.concatenate([first[c], rest[c]]), _expected(rs, name, c), f"after the refusals, cell {c}", 9)
    _check_final(b, name, "after the refusals")
    b.close()
    # scheduler 11: another kernel
    sc = rs.SliceConfig([5] * 4)
    b = rs.BatchScheduler(sc, 25, 4, N_CELLS, sched=rs.RS_SCHED_NVS_NONGREEDY)
    b.seed(SEEDS)
    b.upload_cqi_epochs(synth_cqi(5, (N_CELLS, 1, 20, 25), HIST))
    t0 = b.clock()
    assert L.rs_batch_grant_bound(b._h) == RS_ERR_INVALID and "scheduler 11" in L.rs_last_error().decode()
    assert L.rs_batch_run_grant_records(b._h, 1, 64, recs.ctypes.data, pn) == RS_ERR_INVALID and "scheduler 11" in L.rs_last_error().decode()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(t0, b.clock()))
    b.run(3)
    b.close()
    assert not recs.view(np.uint8).any() and (n == -7).all()


@pytest.mark.gpu
def test_a_queue_model_batch_is_refused(rs, oracle):
    """RS_ERR_STATE, the message points to rs_batch_run_records -- whose own refusal of a batch WITHOUT the queue model stays what it is"""
    import queue_edges as qe
    from test_gpu_queue_edges import _batch as queue_batch, _expected as queue_expected
    p = queue_expected(oracle, "instants")[0]
    b = queue_batch(rs, p)
    L = rs.lib()
    recs = np.zeros((p.n_cells, 8), rs.api.BATCH_GRANT_RECORD)
    n = np.zeros(p.n_cells, np.int64)
    pn = n.ctypes.data_as(L.rs_batch_run_grant_records.argtypes[4])
    t0 = b.clock()
    assert L.rs_batch_grant_bound(b._h) == RS_ERR_STATE and "rs_batch_record_bound" in L.rs_last_error().decode()
    assert L.rs_batch_run_grant_records(b._h, 1, 8, recs.ctypes.data, pn) == RS_ERR_STATE and "rs_batch_run_records" in L.rs_last_error().decode()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(t0, b.clock())) and not recs.view(np.uint8).any()
    assert len(b.run_records(p.n_ttis)) == p.n_cells
    b.close()
    assert qe is not None


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["9-20x5-25x4", "10-20x5-25x4"])
def test_the_self_check_leaves_no_record(rs, oracle, name, monkeypatch):
    """selfcheck = 1 and run_grant_records is the batch's first call: the trial launches on the built-in kernels and on the lean and the
    general records variant write into scratch blocks -- the caller's lists are exact, nothing twice; the plain run that follows is
    self-checked in its own right and the state stays the oracle's."""
    monkeypatch.setenv("RS_JIT_LEAN_MIN_TTIS", "1")
    b = _batch(rs, name, jit=True, selfcheck=1)
    got = b.run_grant_records(20)
    st = b.jit_status()
    assert st[0] == 1 and "agree, state and records" in st[1], st
    assert b.kernel_name == "rs_cell_kernel_jit[lean,records]"
    _check_lists(rs, name, got, f"{name}, self-checked", 0, 20)
    b.run(5)
    assert b.kernel_name == "rs_cell_kernel_jit"
    got = b.run_grant_records(20)
    _check_lists(rs, name, got, f"{name}, self-checked, second call", 25, 45)
    _check_final(b, name, f"{name}, self-checked")
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["9-20x5-25x4", "10-20x5-25x4"])
def test_a_wrong_record_is_caught_by_the_record_comparison(rs, oracle, name, monkeypatch):
    """-DRS_FAULT_INJECT_RECORDS: the run-time builds' RECORD says one byte more than was credited -- the state agrees, only the
    comparison of the record lists can tell.  Lean and general variant are dropped one after the other, the built-in kernels serve the
    call and its records are right; the status names the field; the plain builds are untouched and serve the next plain run."""
    monkeypatch.setenv("RS_JIT_EXTRA", "-DRS_FAULT_INJECT_RECORDS")
    monkeypatch.setenv("RS_JIT_LEAN_MIN_TTIS", "1")
    b = _batch(rs, name, jit=True)
    got = b.run_grant_records(20)
    code, msg = b.jit_status()
    assert code == -2 and "field bytes" in msg and "cell 0, record 0" in msg and "general" in msg, (code, msg)
    assert _builtin_name(b)
    _check_lists(rs, name, got, f"{name}, wrong variants dropped", 0, 20)
    b.run(5)
    assert b.kernel_name == "rs_cell_kernel_jit"     # (the plain builds keep serving)
    got = b.run_grant_records(20)
    assert _builtin_name(b)
    _check_lists(rs, name, got, f"{name}, wrong variants dropped, second call", 25, 45)
    _check_final(b, name, f"{name}, wrong variants dropped")
    b.close()


_MARK_SCRIPT = """
import sys, json
import numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import radiosaber_amd as rs
import test_gpu_batch_grant_records as t
b = t._batch(rs, "9-222-25x4", jit=True)
got = b.run_grant_records(10)
print(json.dumps(dict(status=b.jit_status()[1], kernel=b.kernel_name, stats=rs.jit_cache_stats(), n=[len(g) for g in got],
                      digest=[int(g["bytes"].sum()) for g in got])))
"""


@pytest.mark.gpu
def test_a_second_process_finds_the_mark(rs, tmp_path):
    """The records variant has a cache file and a VERIFIED mark of its own: the first process compiles and checks it, the second loads
    it and skips the check."""
    env = dict(os.environ, RS_JIT_CACHE_DIR=str(tmp_path / "cache"))
    env.pop("RS_JIT_EXTRA", None)
    outs = []
    for _ in range(2):
        r = subprocess.run([sys.executable, "-c", _MARK_SCRIPT.format(root=str(ROOT), tests=str(ROOT / "tests"))], env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    assert "agree, state and records" in outs[0]["status"] and outs[0]["stats"]["misses"] >= 2
    assert "carries the self-check mark" in outs[1]["status"] and outs[1]["stats"]["misses"] == 0 and outs[1]["stats"]["hits"] >= 2
    assert outs[0]["kernel"] == outs[1]["kernel"] == "rs_cell_kernel_jit[records]"
    assert outs[0]["n"] == outs[1]["n"] and outs[0]["digest"] == outs[1]["digest"]


@pytest.mark.gpu
@pytest.mark.parametrize("sched", [9, 7, 1])
def test_run_experiment_writes_the_same_log_from_records(rs, tmp_path, sched):
    """a 20-slice backlogged configuration: the log with --records equals the log of the logged path, byte for byte"""
    cfg = json.loads((GOLDEN / "experiment_configs.json").read_text())["exp-customization/exp-backlogged-20slices/config.json"]
    ref_cfg = {"ues_per_slice": cfg["ues_per_slice"], "slices": [
        dict(n_slices=1, weight=cfg["weight"][s], algo_alpha=cfg["algo_alpha"][s], algo_beta=cfg["algo_beta"][s],
             algo_epsilon=cfg["algo_epsilon"][s], algo_psi=cfg["algo_psi"][s], **cfg["traffic"][s]) for s in range(20)]}
    assert not any(t.get("internet_flow") or t.get("video_app") for t in cfg["traffic"])
    path = tmp_path / "config.json"
    path.write_text(json.dumps(ref_cfg))
    logs = []
    for extra in ([], ["--records"]):
        log = tmp_path / f"sched{sched}{'_records' if extra else ''}.log"
        r = subprocess.run([sys.executable, str(ROOT / "tools" / "run_experiment.py"), "--config", str(path), "--sched", str(sched),
                            "--duration", "0.3", "--log", str(log)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        logs.append(log.read_bytes())
    # (a backlogged configuration keeps scheduler 1's "flow:" line by default, tools/run_experiment.py --sched1-line)
    assert logs[0] == logs[1] and logs[0].count(b"\n") > 300 and (b" flow: " if sched == 1 else b" app: ") in logs[0]
