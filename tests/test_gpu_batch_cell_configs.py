"""Per-cell configurations of a batch (gpu): rs_batch_set_cell_configs gives every cell of one batch its own weights, exponents and slice
sizes, and cell c then runs, to the bit, like a one-cell batch created from row c.

The common set-up is 4 slices, 96 users, 6 RBGs of 2 PRBs, six cells and 90 logged TTIs (the run crosses the CQI refreshes at 40 and
80).  The rows:
  A  [24, 24, 24, 24]  equal weights, PF                    the baseline (and the batch's shared configuration)
  B  [70, 1, 0, 25]                                         a slice above 64 users, a one-user slice, an empty slice
  C  [7, 9, 33, 47]                                         windows straddle multiples of 8; 33 is above the built-in NVS split at 32
  D  [96, 0, 0, 0]     weights .7 .1 .1 .1                  all users in one slice
  E  A's sizes         weights .62 .3 .05 .03, psi 0 (MT)   negative quotas
  F  A's sizes         eps 1 0 1 1, psi 1 1 0 1             mixed exponents per slice
The twins (six one-cell batches on the built-in kernels, same seeds and grids) are run once per (scheduler, grid) and shared."""
import functools
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import synth_cqi
from radiosaber_amd import logfmt
from test_gpu_parity import HIST

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
S, U, R, G, N_TTIS = 4, 96, 6, 2, 90
SCHEDS = [1, 7, 8, 9, 10, 101, 103]
A_SIZES = [24, 24, 24, 24]
ROWS = [  # (sizes, weights, eps, psi)
    (A_SIZES, [0.25] * 4, [1] * 4, [1] * 4),
    ([70, 1, 0, 25], [0.25] * 4, [1] * 4, [1] * 4),
    ([7, 9, 33, 47], [0.25] * 4, [1] * 4, [1] * 4),
    ([96, 0, 0, 0], [0.7, 0.1, 0.1, 0.1], [1] * 4, [1] * 4),
    (A_SIZES, [0.62, 0.3, 0.05, 0.03], [1] * 4, [0] * 4),
    (A_SIZES, [0.25] * 4, [1, 0, 1, 1], [1, 1, 0, 1]),
]
N_CELLS = len(ROWS)
SEEDS = np.arange(N_CELLS, dtype=np.uint32) * 7919 + 805290992
LOG_FIELDS = ("rbg_to_user", "tbs_bits", "quota", "target", "nprb", "final_cqi", "mcs")
STATE_FIELDS = ("avg_rate", "cum_bytes", "cum_rbs", "slice_state")


def _configs(rs):
    return [rs.SliceConfig(list(ues), weight=list(w), algo_epsilon=list(e), algo_psi=list(p)) for ues, w, e, p in ROWS]


@functools.lru_cache(maxsize=None)
def _grids(n_epochs, r=R):
    g = synth_cqi(11, (N_CELLS, n_epochs, U, r), HIST)
    g.setflags(write=False)
    return g


def _batch(rs, sched, configs=None, r=R, g=G, n_epochs=3, **kw):
    """the six-cell batch on these rows (configs=None: the setter is never called), seeded and with its grids"""
    b = rs.BatchScheduler(_configs(rs)[0], r, g, N_CELLS, sched=sched, **kw)
    if configs is not None:
        b.set_cell_configs(configs)
    b.seed(SEEDS)
    b.upload_cqi_epochs(_grids(n_epochs, r))
    return b


_TWINS = {}


def _twins(rs, sched, n_ttis=N_TTIS, logged=True):
    """six one-cell batches on the built-in kernels, one per row: [(logged rows or None, state, clock)], computed once"""
    key = (sched, n_ttis, logged)
    if key not in _TWINS:
        out = []
        n_epochs = (n_ttis + 39) // 40
        for c, cfg in enumerate(_configs(rs)):
            b = rs.BatchScheduler(cfg, R, G, 1, sched=sched)
            b.seed(SEEDS[c:c + 1])
            b.upload_cqi_epochs(_grids(n_epochs)[c:c + 1])
            logs = b.run_logged(n_ttis) if logged else b.run(n_ttis)
            out.append((logs, b.state(), b.clock()))
            b.close()
        _TWINS[key] = out
    return _TWINS[key]


def _same_state(st, c, want, what):
    for f in STATE_FIELDS:
        assert st[f][c].tobytes() == want[f][0].tobytes(), f"{what}: cell {c}, {f} differs from the one-cell batch of its row"


def _same_rows(got, c, want, what):
    for f in LOG_FIELDS:
        np.testing.assert_array_equal(got[f][c], want[f][0], err_msg=f"{what}: cell {c}, {f}")


@pytest.mark.parametrize("sched", SCHEDS)
def test_every_cell_is_the_one_cell_batch_of_its_row(rs, sched):
    b = _batch(rs, sched, _configs(rs))
    got = b.run_logged(N_TTIS)
    st, clock = b.state(), b.clock()
    b.close()
    for c, (logs, want, wclock) in enumerate(_twins(rs, sched)):
        _same_rows(got, c, logs, f"sched {sched}")
        _same_state(st, c, want, f"sched {sched}")
        assert clock[0][c] == wclock[0][0] and clock[1][c] == wclock[1][0]
    if sched != 1:  # (per-flow PF reads neither weights nor slices: its rows differ by seed and grid alone)
        assert any((got["rbg_to_user"][0] != got["rbg_to_user"][c]).any() for c in (1, 2, 3)), "the rows changed nothing"


@pytest.mark.parametrize("sched", [9, 8, 7])
def test_run_time_builds_serve_the_rows(rs, sched):
    """jit=True, selfcheck=1: the general build serves a logged launch, the lean build an unlogged one of 256 TTIs; both against the
    built-in twins, rows and final state."""
    b = _batch(rs, sched, _configs(rs), jit=True, selfcheck=1)
    assert b.jit_status()[0] == 1, b.jit_status()
    got = b.run_logged(N_TTIS)
    assert b.jit_status()[0] == 1 and b.kernel_name == "rs_cell_kernel_jit", b.jit_status()
    st = b.state()
    b.close()
    for c, (logs, want, _) in enumerate(_twins(rs, sched)):
        _same_rows(got, c, logs, f"sched {sched}, general build")
        _same_state(st, c, want, f"sched {sched}, general build")
    n_long = 256
    b = _batch(rs, sched, _configs(rs), n_epochs=7, jit=True, selfcheck=1)
    b.run(n_long)
    status = b.jit_status()
    assert status[0] == 1 and "general and lean" in status[1], status
    st = b.state()
    b.close()
    for c, (_, want, _) in enumerate(_twins(rs, sched, n_long, logged=False)):
        _same_state(st, c, want, f"sched {sched}, lean build")


def test_the_autotune_trials_carry_the_rows(rs):
    """autotune=True: the candidates are timed on the batch's own TTIs, each a build with the rows' switch; the run is the twins' run"""
    n_long = 256
    b = _batch(rs, 8, _configs(rs), n_epochs=7, jit=True, autotune=True, selfcheck=1)
    b.run(n_long)
    n, report = b.autotune_report()
    assert n >= 2 and "REJECTED" not in report and b.jit_status()[0] == 1, (report, b.jit_status())
    st = b.state()
    b.close()
    for c, (_, want, _) in enumerate(_twins(rs, 8, n_long, logged=False)):
        _same_state(st, c, want, "sched 8, autotuned lean build")


def test_a_second_call_replaces_the_first_and_null_keeps_the_shared_values(rs):
    cfgs = _configs(rs)
    b = _batch(rs, 9, cfgs[::-1])
    b.set_cell_configs(cfgs)
    got, st = b.run_logged(N_TTIS), b.state()
    b.close()
    for c, (logs, want, _) in enumerate(_twins(rs, 9)):
        _same_rows(got, c, logs, "second call")
        _same_state(st, c, want, "second call")
    # weights and maps alone: exponents NULL -> the shared configuration's (row A's ones), also over rows set before
    L = rs.lib()
    b = _batch(rs, 9, cfgs)
    w = np.ascontiguousarray([c.weight for c in cfgs], np.float64)
    m = np.ascontiguousarray([c.user_to_slice for c in cfgs], np.int32)
    t = L.rs_batch_set_cell_configs.argtypes
    assert L.rs_batch_set_cell_configs(b._h, w.ctypes.data_as(t[1]), None, None, m.ctypes.data_as(t[4])) == 0, L.rs_last_error()
    for c in range(N_CELLS):
        row = b.cell_config(c)
        np.testing.assert_array_equal(row["weight"], cfgs[c].weight)
        np.testing.assert_array_equal(row["user_to_slice"], cfgs[c].user_to_slice)
        assert (row["algo_epsilon"] == 1).all() and (row["algo_psi"] == 1).all()
    b.close()


def _against_the_oracle(rs, oracle, sched, r, g):
    """tests/test_gpu_parity.py's _check_batch, with a row per cell"""
    grids = _grids(3, r)
    b = _batch(rs, sched, _configs(rs), r=r, g=g)
    got = b.run_logged(N_TTIS)
    st = b.state()
    b.close()
    for c, (ues, w, e, p) in enumerate(ROWS):
        cell = oracle.Cell(list(ues), r, g, sched, weights=list(w), epsilon=list(e), psi=list(p))
        logs = cell.run_synth(grids[c], int(SEEDS[c]), N_TTIS, phy_error_draws=0)
        ost = cell.state()
        np.testing.assert_array_equal(got["rbg_to_user"][c], logs["rbg_to_user"], err_msg=f"cell {c} RBG map")
        np.testing.assert_array_equal(got["tbs_bits"][c], logs["tbs_bits"], err_msg=f"cell {c} TBS")
        np.testing.assert_array_equal(st["cum_bytes"][c], ost["cum_bytes"])
        np.testing.assert_array_equal(st["cum_rbs"][c], ost["cum_rbs"])
        assert st["avg_rate"][c].tobytes() == ost["avg_rate"].tobytes(), f"cell {c} PF averages differ"
        assert st["slice_state"][c].tobytes() == ost["slice_state"].tobytes(), f"cell {c} slice state differs"


@pytest.mark.parametrize("sched", [9, 7])
def test_every_cell_is_the_oracle_of_its_row(rs, oracle, sched):
    _against_the_oracle(rs, oracle, sched, R, G)


def test_the_oracle_at_25_rbgs_of_4(rs, oracle):
    _against_the_oracle(rs, oracle, 9, 25, 4)


@pytest.mark.parametrize("sched", [9, 7])
def test_uniform_rows_change_nothing(rs, sched):
    plain = _batch(rs, sched)
    want, wst = plain.run_logged(N_TTIS), plain.state()
    plain.close()
    b = _batch(rs, sched, [_configs(rs)[0]] * N_CELLS)
    got, st = b.run_logged(N_TTIS), b.state()
    b.close()
    for f in LOG_FIELDS:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f)
    for f in STATE_FIELDS:
        assert st[f].tobytes() == wst[f].tobytes(), f


def _refused(rs, b, code, *words, **arrays):
    L = rs.lib()
    before = [b.cell_config(c) for c in range(N_CELLS)]
    args = [arrays.get(k) for k in ("w", "e", "p", "m")]
    types = (np.float64, np.int32, np.int32, np.int32)
    held = [None if x is None else np.ascontiguousarray(x, t) for x, t in zip(args, types)]
    rc = L.rs_batch_set_cell_configs(b._h, *[None if x is None else x.ctypes.data_as(L.rs_batch_set_cell_configs.argtypes[i + 1]) for i, x in enumerate(held)])
    msg = L.rs_last_error().decode()
    assert rc == code, (rc, msg)
    for w in words:
        assert w in msg, msg
    after = [b.cell_config(c) for c in range(N_CELLS)]
    for x, y in zip(before, after):
        assert all(x[k].tobytes() == y[k].tobytes() for k in x), "a refused call changed a row"


def test_refusals(rs):
    INVALID, STATE = -1, -4
    cfgs = _configs(rs)
    maps = np.stack([c.user_to_slice for c in cfgs])
    ws = np.array([c.weight for c in cfgs])
    # invalid rows name the cell; nothing is stored (once on a fresh batch, once over rows that were set)
    for preset in (False, True):
        b = _batch(rs, 9, cfgs if preset else None)
        bad = maps.copy(); bad[2, 50] = 0
        _refused(rs, b, INVALID, "cell 2", "user 50", m=bad)                # a decreasing map
        bad = maps.copy(); bad[4, 95] = S
        _refused(rs, b, INVALID, "cell 4", "user 95", m=bad)                # a slice id of S
        bad = np.ones((N_CELLS, S), np.int32); bad[3, 1] = 2
        _refused(rs, b, INVALID, "cell 3", "slice 1", e=bad)                # eps = 2
        bad = ws.copy(); bad[5, 2] = np.nan
        _refused(rs, b, INVALID, "cell 5", "[2]", w=bad)                    # a NaN weight
        bad = ws.copy(); bad[1] = 600.0                                     # 5 * 12 PRBs * (1 + 2400) >= 2^15
        _refused(rs, b, INVALID, "cell 1", "32768", w=bad)                  # weights outside the slice-state domain
        want = cfgs if preset else [cfgs[0]] * N_CELLS
        for c in range(N_CELLS):
            got = b.cell_config(c)
            np.testing.assert_array_equal(got["user_to_slice"], want[c].user_to_slice)
            np.testing.assert_array_equal(got["weight"], want[c].weight)
            np.testing.assert_array_equal(got["algo_epsilon"], want[c].algo_epsilon)
            np.testing.assert_array_equal(got["algo_psi"], want[c].algo_psi)
        # after a run: the rows stay what they were
        b.run(5)
        _refused(rs, b, STATE, "after TTIs", m=maps)
        b.close()
    # the queue model, in either order
    b = rs.BatchScheduler(cfgs[0], R, G, N_CELLS, sched=9)
    b.set_bearers(cfgs[0].bearer_kinds())
    _refused(rs, b, STATE, "queue model", m=maps)
    b.close()
    b = rs.BatchScheduler(cfgs[0], R, G, N_CELLS, sched=9)
    b.set_cell_configs(cfgs)
    with pytest.raises(rs.RadioSaberError) as err:
        b.set_bearers(cfgs[0].bearer_kinds())
    assert err.value.code == STATE
    assert "rs_batch_set_cell_configs" in str(err.value)
    b.close()
    # scheduler 11
    b = rs.BatchScheduler(cfgs[0], R, G, N_CELLS, sched=11)
    _refused(rs, b, INVALID, "scheduler 11", m=maps)
    b.close()


@pytest.mark.parametrize("preset", [True, False])
def test_reducers(rs, preset):
    cfgs = _configs(rs)
    b = _batch(rs, 9, cfgs if preset else None)
    b.run(N_TTIS)
    st, tot, by = b.state(), b.slice_totals(), b.slice_bytes()
    b.close()
    assert st["cum_bytes"].sum() > 0
    for c in range(N_CELLS):
        m = (cfgs[c] if preset else cfgs[0]).user_to_slice
        for f in ("cum_bytes", "cum_rbs"):
            want = np.array([st[f][c][m == s].sum() for s in range(S)], np.int64)
            np.testing.assert_array_equal(tot[f][c], want, err_msg=f"cell {c} {f}")
    np.testing.assert_array_equal(by.astype(np.int64), tot["cum_bytes"].sum(axis=0))


def test_checkpoint(rs):
    cfgs = _configs(rs)
    whole = _batch(rs, 9, cfgs)
    whole.run(120)
    want = whole.state()
    whole.close()
    first = _batch(rs, 9, cfgs)
    first.run(60)
    blob = first.checkpoint()
    first.close()
    second = _batch(rs, 9, cfgs)
    second.restore(blob)
    second.run(60)
    got = second.state()
    second.close()
    for f in STATE_FIELDS:
        assert got[f].tobytes() == want[f].tobytes(), f
    # other rows (cells E and F swapped), and no rows at all: refused
    other = _batch(rs, 9, cfgs[:4] + [cfgs[5], cfgs[4]])
    with pytest.raises(rs.RadioSaberError) as err:
        other.restore(blob)
    assert "configured differently" in str(err.value)
    other.close()
    plain = _batch(rs, 9)
    with pytest.raises(rs.RadioSaberError):
        plain.restore(blob)
    plain.close()


@pytest.mark.parametrize("sched", [9, 10])
def test_grant_records(rs, sched):
    cfgs = _configs(rs)
    b = _batch(rs, sched, cfgs)
    bound = b.grant_bound()
    recs = b.run_grant_records(N_TTIS)
    st = b.state()
    b.close()
    per_cell = [sum(min(n, R) for n in c.ues_per_slice) if sched == 10 else min(U, R) for c in cfgs]
    assert bound == max(per_cell) and (sched != 10 or bound > min(per_cell))
    for c, (logs, want, _) in enumerate(_twins(rs, sched)):
        uinfo = logs["nprb"][0] | (logs["final_cqi"][0] << 16) | (logs["mcs"][0] << 24)
        exp = logfmt.grant_records_from_rows(logs["tbs_bits"][0], uinfo, None if sched == 10 else logs["rbg_to_user"][0])
        mine = recs[c].copy()
        if sched == 10:  # (two users of different slices may hold one RBG: the map cannot give UpperBound's masks)
            mine["rbg_mask"] = 0
        assert len(mine) == len(exp) and mine.tobytes() == exp.astype(mine.dtype).tobytes(), f"cell {c}"
        _same_state(st, c, want, f"sched {sched}, records launch")


def _ref_config(sizes, w, e, p):
    return {"ues_per_slice": list(sizes), "slices": [dict(n_slices=1, weight=w[s], algo_alpha=0, algo_beta=0, algo_epsilon=e[s], algo_psi=p[s])
                                                     for s in range(len(sizes))]}


def test_run_experiment_runs_configs_times_seeds_as_one_batch(rs, tmp_path):
    """two configurations x two seeds through tools/run_experiment.py: four logs, each byte for byte the log of its single run"""
    tool = [sys.executable, str(ROOT / "tools" / "run_experiment.py"), "--sched", "9", "--duration", "0.12", "--nb-rbs", "12", "--rbg-size", "2"]
    names = {"config-pf": ROWS[2], "config-mt": ROWS[4]}
    for name, row in names.items():
        (tmp_path / f"{name}.json").write_text(json.dumps(_ref_config(*row)))
    r = subprocess.run(tool + ["--config"] + [str(tmp_path / f"{n}.json") for n in names] + ["--seeds", "0,3", "--log", str(tmp_path / "batch_{config}_{seed}.log")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    logs = set()
    for name in names:
        for seed in (0, 3):
            single = tmp_path / f"single_{name}_{seed}.log"
            r = subprocess.run(tool + ["--config", str(tmp_path / f"{name}.json"), "--seed", str(seed), "--log", str(single)], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr[-2000:]
            got = (tmp_path / f"batch_{name}_{seed}.log").read_bytes()
            assert got == single.read_bytes() and got.count(b"\n") > 100, (name, seed)
            logs.add(got)
    assert len(logs) == 4
