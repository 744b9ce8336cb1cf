"""GPU: bearer records of unlogged queue-model launches (rs_batch_run_records) -- one 32-byte record per bearer DoStopSchedule credits,
exact against the oracle's run and against logged twins.

The expected records are what the stepped oracle (queue_edges.oracle_run: rso_cell_step_queues) implies: the non-zero entries of its
bearer_bytes, bearer_hol bitwise, the PRBs as the step of cum_rbs; in BearerLogWriter's order (TTI, user, then bearer 1 before 0, or 0
before 1 for scheduler 1).  PARITY UNPINNED like the queue model itself (tests/PINS.md)."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import queue_edges as qe
from conftest import GOLDEN, synth_cqi
from radiosaber_amd import logfmt
from test_gpu_flow_log import HIST, _customize_case
from test_gpu_queue_edges import LOGGED, _batch, _check_final, _expected

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
RS_ERR_INVALID, RS_ERR_STATE, RS_ERR_RANGE = -1, -4, -5


def _records_of(rs, sched, by, hol, rbs, t0=0):
    """[T][U][2] credited bytes, HoL delays and PRBs of one cell -> its records in the writer's order, TTIs counted from t0"""
    rows = []
    for n, u in np.argwhere(np.asarray(by).any(2)):
        for k in ((0, 1) if sched == 1 else (1, 0)):
            if by[n, u, k] > 0:
                rows.append((t0 + n, u, k, by[n, u, k], rbs[n, u, k], 0, hol[n, u, k]))
    return np.array(rows, rs.api.BEARER_RECORD)


def _oracle_records(rs, p, run, c, t0=0, t1=None):
    """the oracle's records of cell c in TTIs t0 .. t1 - 1"""
    t1 = p.n_ttis if t1 is None else t1
    rbs = np.diff(np.concatenate([np.zeros_like(run["cum_rbs"][c, :1]), run["cum_rbs"][c]]), axis=0)
    return _records_of(rs, p.sched, run["bearer_bytes"][c, t0:t1], run["bearer_hol"][c, t0:t1], rbs[t0:t1], t0)


def _same(got, want, what):
    assert got.dtype == want.dtype and len(got) == len(want), f"{what}: {len(got)} records against {len(want)}"
    bad = np.flatnonzero(got != want)[:3]   # (0.0 == -0.0 and NaN never occur here; the bytes decide)
    assert got.tobytes() == want.tobytes(), f"{what}: first differences {[(got[i], want[i]) for i in bad]}"


def _checkpoint_state(b):
    """The batch's checkpoint block without the diagnostics it carries along: the last 32 bytes of every cell's 240-byte scalar record
    are the last launch's first and last instruction on the shader and the 100 MHz clock (rs_batch_debug_clocks), which no two
    launches share.  The block is a header, then [cells][U] averages (8), pending grants (4), bytes and RBs (8 each), [cells][S] slice
    state (8), the scalar records, then the queue model's parts."""
    blob = bytearray(b.checkpoint())
    cells, U, S = b.n_cells, b.U, b.S
    ahead = 28 * cells * U + 8 * cells * S
    behind = 240 * cells + (28 + 8 + 16) * 2 * cells * U + 9 * cells * U
    scal = len(blob) - behind
    assert scal - ahead == 64, "the checkpoint's layout is not the one this helper masks"
    for c in range(cells):
        blob[scal + 240 * c + 208:scal + 240 * (c + 1)] = bytes(32)
    return bytes(blob)


@pytest.mark.parametrize("variant", [v[0] for v in LOGGED])
@pytest.mark.parametrize("family", list(qe.FAMILY_CELLS))
def test_records_of_the_edge_populations(rs, oracle, family, variant):
    p, run, _, _, done = _expected(oracle, family)
    what = f"{family}, {variant}"
    b = _batch(rs, p, **dict(LOGGED)[variant])
    assert b.record_bound() == (min(2 * p.n_users, p.R) if p.sched == 1 else 2 * min(p.n_users, p.R))
    got = b.run_records(p.n_ttis)
    if variant != "built-in":
        assert b.jit_status()[0] == 1, b.jit_status()
    assert len(got) == p.n_cells
    for c in range(p.n_cells):
        _same(got[c], _oracle_records(rs, p, run, c), f"{what}, cell {c}")
    _check_final(rs, p, run, done, b, what)
    b.close()


@pytest.mark.parametrize("family", list(qe.FAMILY_CELLS))
def test_records_of_the_lean_build(rs, oracle, family, monkeypatch):
    monkeypatch.setenv("RS_JIT_LEAN_MIN_TTIS", "1")
    p, run, _, _, done = _expected(oracle, family)
    b = _batch(rs, p, jit=True)
    got = b.run_records(p.n_ttis)
    assert b.jit_status()[0] == 1 and "unavailable" not in b.jit_status()[1], b.jit_status()
    for c in range(p.n_cells):
        _same(got[c], _oracle_records(rs, p, run, c), f"{family}, lean build, cell {c}")
    _check_final(rs, p, run, done, b, f"{family}, lean build")
    b.close()


@pytest.mark.parametrize("split", ["one-tti-launches", "two-unequal-launches"])
@pytest.mark.parametrize("variant", [v[0] for v in LOGGED])
@pytest.mark.parametrize("family", ["instants", "split-QQ"])
def test_split_launches_concatenate(rs, oracle, family, variant, split):
    """Every pending DoStopSchedule crosses a launch boundary: the record belongs to the launch that credits it, its tti goes on counting."""
    p, run, _, _, done = _expected(oracle, family)
    launches = [1] * p.n_ttis if split == "one-tti-launches" else [1, p.n_ttis - 1] if p.n_ttis < 8 else [p.n_ttis // 3, p.n_ttis - p.n_ttis // 3]
    b = _batch(rs, p, **dict(LOGGED)[variant])
    parts, t0 = [], 0
    for n in launches:
        got = b.run_records(n)
        for c in range(p.n_cells):
            _same(got[c], _oracle_records(rs, p, run, c, t0, t0 + n), f"{family}, {variant}, TTIs {t0} .. {t0 + n - 1}, cell {c}")
        parts.append(got)
        t0 += n
    for c in range(p.n_cells):
        _same(np.concatenate([g[c] for g in parts]), _oracle_records(rs, p, run, c), f"{family}, {variant}, {split}, cell {c}")
    _check_final(rs, p, run, done, b, f"{family}, {variant}, {split}")
    b.close()


@pytest.mark.parametrize("variant", [v[0] for v in LOGGED])
def test_twins_on_split_BQ(rs, oracle, variant):
    """run_records IS run: a batch that ran one and a batch that ran the other cannot be told apart; and the records are the non-zero
    rows of a logged launch."""
    p, run, _, _, _ = _expected(oracle, "split-BQ")
    kw = dict(LOGGED)[variant]
    a, b, c3 = _batch(rs, p, **kw), _batch(rs, p, **kw), _batch(rs, p, **kw)
    size0 = len(a.checkpoint())
    recs = a.run_records(p.n_ttis)
    b.run(p.n_ttis)
    assert len(a.checkpoint()) == size0 == len(b.checkpoint())
    for key, v in a.state().items():
        assert v.tobytes() == b.state()[key].tobytes(), f"{variant}: state {key}"
    for key, v in a.bearer_state().items():
        assert v.tobytes() == b.bearer_state()[key].tobytes(), f"{variant}: bearer state {key}"
    ra, rb = a.flow_record(), b.flow_record()
    assert ra.keys() == rb.keys() and all(ra[k][0].tobytes() == rb[k][0].tobytes() and ra[k][1].tobytes() == rb[k][1].tobytes() for k in ra)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a.clock(), b.clock()))
    assert _checkpoint_state(a) == _checkpoint_state(b), f"{variant}: the checkpoint blocks differ"
    got = c3.run_logged(p.n_ttis, bearers=True)
    for c in range(p.n_cells):
        rbs = logfmt.bearer_prbs(got["rbg_to_user"][c], got["nprb"][c], p.G, pf_flows=p.sched == 1)
        _same(recs[c], _records_of(rs, p.sched, got["bearer_bytes"][c], got["bearer_hol"][c], rbs), f"{variant}, cell {c}: records against logged rows")
    for x in (a, b, c3):
        x.close()


@pytest.mark.parametrize("threads", [64, 0])
@pytest.mark.parametrize("sched", [1, 7, 9])
def test_several_users_per_thread(rs, sched, threads):
    """The customised-slice shape, 194 UEs on 64 RBGs: with 64 threads four trips of the user loop, the last one partial; with the
    default the grants lie in several waves (run-time build: the launch's counters ride in registers).  Records == the non-zero rows of a
    logged twin, record_lines == lines, and no cell-TTI exceeds the bound."""
    n_cells, n_ttis = 2, 200
    sc, kinds, bursts, R, G = _customize_case(rs, n_cells, n_ttis)
    grids = synth_cqi(31 + sched, (n_cells, (n_ttis + 39) // 40, sc.n_users, R), HIST)
    seeds = np.array([41, 42], np.uint32)

    def batch():
        b = rs.BatchScheduler(sc, R, G, n_cells, sched=sched, threads_per_cell=threads, jit=threads == 0)
        b.set_bearers(kinds)
        b.set_arrivals(bursts)
        b.seed(seeds)
        b.upload_cqi_epochs(grids)
        return b

    a, b = batch(), batch()
    t_first = a.clock()[0].copy()
    bound = a.record_bound()
    assert bound == (64 if sched == 1 else 128)
    recs = a.run_records(n_ttis)
    got = b.run_logged(n_ttis, bearers=True)
    done_a, done_b = a.flow_record(), b.flow_record()
    app_of, ipflow = logfmt.app_ids(sc), logfmt.internet_flow_bearers(sc)
    total = 0
    for c in range(n_cells):
        rbs = logfmt.bearer_prbs(got["rbg_to_user"][c], got["nprb"][c], G, pf_flows=sched == 1)
        _same(recs[c], _records_of(rs, sched, got["bearer_bytes"][c], got["bearer_hol"][c], rbs), f"sched {sched}, {threads} threads, cell {c}")
        per_tti = np.bincount(recs[c]["tti"], minlength=n_ttis)
        assert len(per_tti) == n_ttis and per_tti.max() <= bound, (per_tti.max(), bound)
        total += len(recs[c])
        flows = {(u, k): v for (cc, u, k), v in bursts.items() if cc == c and ipflow[u, k]}
        wa = logfmt.BearerLogWriter(app_of, sc.user_to_slice, pf_flows=sched == 1, flows=flows)
        wb = logfmt.BearerLogWriter(app_of, sc.user_to_slice, pf_flows=sched == 1, flows=flows)
        want = wb.lines(got["bearer_bytes"][c], got["bearer_hol"][c], rbs, float(t_first[c]), {(u, k): v for (cc, u, k), v in done_b.items() if cc == c})
        mine = wa.record_lines(recs[c], float(t_first[c]), n_ttis, {(u, k): v for (cc, u, k), v in done_a.items() if cc == c})
        assert mine == want and any(ln.startswith("ipflow end") for ln in want)
    assert total > n_cells * n_ttis   # (more than one credited bearer per cell-TTI: places are handed out to several threads at once)
    a.close()
    b.close()


def test_overflow(rs, oracle):
    """`instants`, four TTIs, cap = record_bound() = 4: the oracle credits 3, 3, 7 and 5 bearers in the four cells."""
    p, run, _, _, _ = _expected(oracle, "instants")
    n = 4
    want = [_oracle_records(rs, p, run, c, 0, n) for c in range(p.n_cells)]
    a, b = _batch(rs, p), _batch(rs, p)
    cap = a.record_bound()
    over = [c for c in range(p.n_cells) if len(want[c]) > cap]
    assert over and len(over) < p.n_cells, [len(w) for w in want]
    with pytest.raises(rs.RadioSaberError) as e:
        a.run_records(n, cap=cap)
    assert e.value.code == RS_ERR_RANGE and f"cell {over[0]} " in str(e.value), str(e.value)
    assert e.value.counts.tolist() == [len(w) for w in want]
    for c in range(p.n_cells):
        if c not in over:
            _same(e.value.records[c], want[c], f"cell {c}, within the capacity")
        else:   # (nothing at or behind the capacity; what was written is a record of the list)
            assert len(e.value.records[c]) == cap
            assert all(any(r.tobytes() == w.tobytes() for w in want[c]) for r in e.value.records[c])
    b.run(n)
    for key, v in a.state().items():
        assert v.tobytes() == b.state()[key].tobytes(), key
    for key, v in a.bearer_state().items():
        assert v.tobytes() == b.bearer_state()[key].tobytes(), key
    assert _checkpoint_state(a) == _checkpoint_state(b)
    nxt = a.run_records(p.n_ttis - n)
    for c in range(p.n_cells):
        _same(nxt[c], _oracle_records(rs, p, run, c, n, p.n_ttis), f"cell {c}, the call after the overflow")
    a.close()
    b.close()


def test_refusals_launch_nothing(rs, oracle):
    """Every refusal is checked before anything is launched: clock and state as they were.  (RS_ERR_HIP, the device block that cannot
    be allocated: test_a_refused_allocation below.)"""
    p, _, _, _, _ = _expected(oracle, "instants")
    b = _batch(rs, p)
    b.run(2)
    L = rs.lib()
    recs = np.zeros((p.n_cells, 8), rs.api.BEARER_RECORD)
    n = np.zeros(p.n_cells, np.int64)
    pn = n.ctypes.data_as(L.rs_batch_run_records.argtypes[4])
    before = (b.clock(), b.state(), b.checkpoint())
    for args, code, word in (((1, 8, None, pn), RS_ERR_INVALID, "null"), ((1, 8, recs.ctypes.data, None), RS_ERR_INVALID, "null"),
                             ((1, 0, recs.ctypes.data, pn), RS_ERR_INVALID, "cap"), ((1, -3, recs.ctypes.data, pn), RS_ERR_INVALID, "cap"),
                             ((0, 8, recs.ctypes.data, pn), RS_ERR_INVALID, "n_ttis"), ((-1, 8, recs.ctypes.data, pn), RS_ERR_INVALID, "n_ttis"),
                             ((32769, 8, recs.ctypes.data, pn), RS_ERR_INVALID, "32768")):
        assert L.rs_batch_run_records(b._h, *args) == code, args
        assert word in L.rs_last_error().decode(), (args, L.rs_last_error().decode())
    after = (b.clock(), b.state(), b.checkpoint())
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before[0], after[0]))
    assert all(before[1][k].tobytes() == after[1][k].tobytes() for k in before[1]) and before[2] == after[2]
    assert not recs.view(np.uint8).any() and not n.any()
    b.close()
    # no queue model: both calls are RS_ERR_STATE
    sc = rs.SliceConfig(p.ues)
    b = rs.BatchScheduler(sc, p.R, p.G, p.n_cells, sched=p.sched)
    b.seed(p.seeds())
    b.upload_cqi_epochs(p.grids())
    t0 = b.clock()
    assert L.rs_batch_record_bound(b._h) == RS_ERR_STATE and "queue model" in L.rs_last_error().decode()
    assert L.rs_batch_run_records(b._h, 1, 8, recs.ctypes.data, pn) == RS_ERR_STATE and "queue model" in L.rs_last_error().decode()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(t0, b.clock()))
    b.close()
    # bearers without arrivals: the queue model is not complete
    b = rs.BatchScheduler(rs.SliceConfig(p.ues, algo_alpha=p.alpha or [], algo_beta=p.beta or []), p.R, p.G, p.n_cells, sched=p.sched)
    b.set_bearers(p.kind_codes())
    b.seed(p.seeds())
    b.upload_cqi_epochs(p.grids())
    assert L.rs_batch_run_records(b._h, 1, 8, recs.ctypes.data, pn) == RS_ERR_STATE
    b.close()
    # the queue model without a CQI source: the launch's own refusal, as from rs_batch_run; nothing is launched
    b = rs.BatchScheduler(rs.SliceConfig(p.ues, algo_alpha=p.alpha or [], algo_beta=p.beta or []), p.R, p.G, p.n_cells, sched=p.sched)
    b.set_bearers(p.kind_codes())
    b.set_arrivals(p.bursts)
    b.seed(p.seeds())
    t0 = b.clock()
    assert L.rs_batch_run_records(b._h, 1, 8, recs.ctypes.data, pn) == RS_ERR_STATE and "CQI" in L.rs_last_error().decode()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(t0, b.clock())) and not recs.view(np.uint8).any() and not n.any()
    b.close()


def test_a_refused_allocation(rs, oracle, monkeypatch):
    """RS_ERR_HIP: the device block cannot be allocated.  RS_RECORDS_MAX_BYTES makes a block above it a failed allocation by the very
    path of one (the old block is freed first, the batch is left without one), so no card is asked for memory it does not have.
    `instants`: 4 cells, bound 4 -- a call of n TTIs needs 4 * 4 n records of 32 bytes and 4 count words.  Nothing is launched, the
    batch does not move, the caller's arrays are not written; the next call allocates again and is exact."""
    p, run, _, _, done = _expected(oracle, "instants")
    b = _batch(rs, p)
    L = rs.lib()
    small = p.n_cells * 2 * b.record_bound() * 32 + 4 * p.n_cells
    got = b.run_records(2)                                  # (a block of `small` bytes exists now)
    for c in range(p.n_cells):
        _same(got[c], _oracle_records(rs, p, run, c, 0, 2), f"cell {c}, TTIs 0 .. 1")
    monkeypatch.setenv("RS_RECORDS_MAX_BYTES", str(small))
    before = (b.clock(), b.state(), b.bearer_state(), b.checkpoint())
    cap = 4 * b.record_bound()
    recs = np.zeros((p.n_cells, cap), rs.api.BEARER_RECORD)
    n = np.full(p.n_cells, -7, np.int64)
    for _ in range(2):                                      # (the second time there is no old block to free)
        rc = L.rs_batch_run_records(b._h, 4, cap, recs.ctypes.data, n.ctypes.data_as(L.rs_batch_run_records.argtypes[4]))
        assert rc == -3 and "no device block of" in L.rs_last_error().decode(), (rc, L.rs_last_error().decode())
        assert (n == -7).all() and not recs.view(np.uint8).any()
    with pytest.raises(rs.RadioSaberError) as e:
        b.run_records(4)
    assert e.value.code == -3
    after = (b.clock(), b.state(), b.bearer_state(), b.checkpoint())
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before[0], after[0])) and before[3] == after[3]
    assert all(before[i][k].tobytes() == after[i][k].tobytes() for i in (1, 2) for k in before[i])
    got = b.run_records(2)                                  # fits the limit: allocated again
    for c in range(p.n_cells):
        _same(got[c], _oracle_records(rs, p, run, c, 2, 4), f"cell {c}, the call after the refusal")
    monkeypatch.delenv("RS_RECORDS_MAX_BYTES")
    got = b.run_records(p.n_ttis - 4)                       # grows
    for c in range(p.n_cells):
        _same(got[c], _oracle_records(rs, p, run, c, 4, p.n_ttis), f"cell {c}, the rest")
    _check_final(rs, p, run, done, b, "after a refused allocation")
    b.close()


@pytest.mark.parametrize("family", ["instants", "gate1-25x4"])
def test_the_self_check_leaves_no_record(rs, oracle, family, monkeypatch):
    """jit, selfcheck = 1, and the batch's first call is run_records: the trial launches of the built-in kernels, the general and the
    lean build run ahead of the real launch and write no record -- the lists are exact, nothing twice."""
    monkeypatch.setenv("RS_JIT_LEAN_MIN_TTIS", "1")
    p, run, _, _, done = _expected(oracle, family)
    b = _batch(rs, p, jit=True, selfcheck=1)
    got = b.run_records(p.n_ttis)
    st = b.jit_status()
    assert st[0] == 1 and "agree" in st[1], st
    for c in range(p.n_cells):
        _same(got[c], _oracle_records(rs, p, run, c), f"{family}, self-checked, cell {c}")
    _check_final(rs, p, run, done, b, f"{family}, self-checked")
    b.close()


@pytest.mark.parametrize("sched", [1, 7, 9])
def test_run_experiment_writes_the_same_log_from_records(rs, tmp_path, sched):
    cfg = json.loads((GOLDEN / "experiment_configs.json").read_text())["exp-customization/exp-customize-20slices/config.json"]
    ref_cfg = {"ues_per_slice": cfg["ues_per_slice"], "slices": [
        dict(n_slices=1, weight=cfg["weight"][s], algo_alpha=cfg["algo_alpha"][s], algo_beta=cfg["algo_beta"][s],
             algo_epsilon=cfg["algo_epsilon"][s], algo_psi=cfg["algo_psi"][s], **cfg["traffic"][s]) for s in range(20)]}
    path = tmp_path / "config.json"
    path.write_text(json.dumps(ref_cfg))
    logs = []
    for extra in ([], ["--records"]):
        log = tmp_path / f"sched{sched}{'_records' if extra else ''}.log"
        r = subprocess.run([sys.executable, str(ROOT / "tools" / "run_experiment.py"), "--config", str(path), "--sched", str(sched),
                            "--duration", "0.3", "--log", str(log)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        logs.append(log.read_bytes())
    assert logs[0] == logs[1] and logs[0].count(b"\n") > 300 and b"ipflow end" in logs[0]
