"""Cells of different user counts in one batch (gpu): a cell's row of user_to_slice may end in RS_USER_ABSENT, and cell c then runs, to
the bit, like a one-cell batch of its n_c users, while the absent users behind them are never scanned, never granted and never written.

The common set-up is tests/test_gpu_batch_cell_configs.py's: 4 slices, 96 users, 6 RBGs of 2 PRBs, 90 logged TTIs (across the CQI
refreshes at 40 and 80), explicit grids.  The rows (slice sizes -> n_c):
  A  [24, 24, 24, 24]  96  a full cell in a ragged batch
  B  [7, 9, 33, 12]    61  the last window ends off a multiple of 8; unequal weights, psi = 0 on one slice
  C  [10, 10, 10, 10]  40  ends on a multiple of 8
  D  [1, 0, 0, 0]       1  a single user
  E  [20, 30, 0, 0]    50  trailing empty slices; unequal weights, psi = 0 on one slice
  F  [24, 24, 24, 23]  95  one absent user
  G  [65, 0, 0, 0]     65  one slice across a wave boundary; for scheduler 1 a count that is no multiple of 32
The bait: every absent user reports CQI 15 on every RBG in every epoch, its PF average is 1.25 (next to the clamp at 1: with CQI 15 its
metric leads) and its cumulative counters hold recognisable values: a leaked user wins RBGs, a touched word shows.  The counters have
no setter of their own, so they come in through a checkpoint of the batch itself, taken before the first TTI.
The twins (seven one-cell batches of n_c users on the built-in kernels, same seeds, the first n_c rows of the grids) are run once per
(scheduler, length) and shared."""
import functools
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import synth_cqi
from test_gpu_parity import HIST

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
S, U, R, G, N_TTIS = 4, 96, 6, 2, 90
SCHEDS = [1, 7, 8, 9, 10, 101, 103]
ROWS = [  # (sizes, weights, eps, psi)
    ([24, 24, 24, 24], [0.25] * 4, [1] * 4, [1] * 4),
    ([7, 9, 33, 12], [0.4, 0.3, 0.2, 0.1], [1] * 4, [1, 1, 0, 1]),
    ([10, 10, 10, 10], [0.25] * 4, [1] * 4, [1] * 4),
    ([1, 0, 0, 0], [0.25] * 4, [1] * 4, [1] * 4),
    ([20, 30, 0, 0], [0.6, 0.2, 0.1, 0.1], [1] * 4, [1, 0, 1, 1]),
    ([24, 24, 24, 23], [0.25] * 4, [1] * 4, [1] * 4),
    ([65, 0, 0, 0], [0.25] * 4, [1] * 4, [1] * 4),
]
N_CELLS = len(ROWS)
NC = [sum(r[0]) for r in ROWS]
SEEDS = np.arange(N_CELLS, dtype=np.uint32) * 7919 + 805290992
LOG_FIELDS = ("rbg_to_user", "tbs_bits", "quota", "target", "nprb", "final_cqi", "mcs")
USER_LOG_FIELDS = ("tbs_bits", "nprb", "final_cqi", "mcs")   # [cells][TTIs][U]
USER_STATE = ("avg_rate", "cum_bytes", "cum_rbs")
BAIT_AVG, BAIT_BYTES, BAIT_RBS = 1.25, 0x0123456789ABCDE, 0x0FEDCBA98765


def _configs(rs):
    return [rs.SliceConfig(list(ues), weight=list(w), algo_epsilon=list(e), algo_psi=list(p)) for ues, w, e, p in ROWS]


def _full(rs):
    """the batch's shared configuration: row A"""
    return _configs(rs)[0]


@functools.lru_cache(maxsize=None)
def _grids(n_epochs, r=R):
    g = synth_cqi(11, (N_CELLS, n_epochs, U, r), HIST)
    for c, n in enumerate(NC):
        g[c, :, n:, :] = 15   # the bait
    g.setflags(write=False)
    return g


def _bait(b):
    """the absent users' averages through write_state, their counters through a checkpoint of the batch itself (no TTI run yet: the
    block is header, averages, pending grants, cum_bytes, cum_rbs, ... -- rs_batch_checkpoint_save); returns the baited state"""
    st = b.state()
    for c, n in enumerate(NC):
        st["avg_rate"][c, n:] = BAIT_AVG
    avg = st["avg_rate"].copy()
    b.write_state(avg_rate=avg)
    blob = bytearray(b.checkpoint())
    marker = np.ascontiguousarray(avg, np.float64).tobytes()
    off = bytes(blob).find(marker)
    assert off > 0 and bytes(blob).find(marker, off + 1) < 0
    off_cumb = off + (8 + 4) * N_CELLS * U
    cumb = np.zeros((N_CELLS, U), np.int64)
    cumr = np.zeros((N_CELLS, U), np.int64)
    for c, n in enumerate(NC):
        cumb[c, n:] = BAIT_BYTES + np.arange(U - n)
        cumr[c, n:] = BAIT_RBS + np.arange(U - n)
    blob[off_cumb:off_cumb + 8 * N_CELLS * U] = cumb.tobytes()
    blob[off_cumb + 8 * N_CELLS * U:off_cumb + 16 * N_CELLS * U] = cumr.tobytes()
    b.restore(bytes(blob))
    st = b.state()
    np.testing.assert_array_equal(st["cum_bytes"], cumb)
    np.testing.assert_array_equal(st["cum_rbs"], cumr)
    return st


def _batch(rs, sched, configs, r=R, g=G, n_epochs=3, bait=True, **kw):
    b = rs.BatchScheduler(_full(rs), r, g, N_CELLS, sched=sched, **kw)
    b.set_cell_configs(configs)
    b.seed(SEEDS)
    b.upload_cqi_epochs(_grids(n_epochs, r))
    return (b, _bait(b)) if bait else (b, None)


_TWINS = {}


def _twins(rs, sched, n_ttis=N_TTIS, logged=True, records=False):
    """one-cell batches of n_c users on the built-in kernels, one per row: [(rows / records / None, state, clock)], computed once"""
    key = (sched, n_ttis, logged, records)
    if key not in _TWINS:
        out = []
        n_epochs = (n_ttis + 39) // 40
        for c, cfg in enumerate(_configs(rs)):
            b = rs.BatchScheduler(cfg, R, G, 1, sched=sched)
            b.seed(SEEDS[c:c + 1])
            b.upload_cqi_epochs(np.ascontiguousarray(_grids(n_epochs)[c:c + 1, :, :NC[c]]))
            if records:
                logs = (b.grant_bound(), b.run_grant_records(n_ttis)[0].copy())
            else:
                logs = b.run_logged(n_ttis) if logged else b.run(n_ttis)
            out.append((logs, b.state(), b.clock()))
            b.close()
        _TWINS[key] = out
    return _TWINS[key]


def _same_state(st, c, want, what, before):
    n = NC[c]
    for f in USER_STATE:
        assert st[f][c, :n].tobytes() == want[f][0].tobytes(), f"{what}: cell {c}, {f} differs from the one-cell batch of its {n} users"
        assert st[f][c, n:].tobytes() == before[f][c, n:].tobytes(), f"{what}: cell {c}, {f} of an absent user was touched"
    assert st["slice_state"][c].tobytes() == want["slice_state"][0].tobytes(), f"{what}: cell {c}, slice state"


def _same_rows(got, c, want, what):
    n = NC[c]
    for f in LOG_FIELDS:
        if f in USER_LOG_FIELDS:
            np.testing.assert_array_equal(got[f][c][:, :n], want[f][0], err_msg=f"{what}: cell {c}, {f}")
            assert not got[f][c][:, n:].any(), f"{what}: cell {c}, {f}: an absent user's row is not an unserved user's"
        else:
            np.testing.assert_array_equal(got[f][c], want[f][0], err_msg=f"{what}: cell {c}, {f}")
    assert (got["rbg_to_user"][c] < n).all(), f"{what}: cell {c}: an RBG went to an absent user"


@pytest.mark.parametrize("sched", SCHEDS)
def test_every_cell_is_the_one_cell_batch_of_its_users(rs, sched):
    b, before = _batch(rs, sched, _configs(rs))
    np.testing.assert_array_equal(b.cell_users(), NC)
    got = b.run_logged(N_TTIS)
    st, clock = b.state(), b.clock()
    b.close()
    for c, (logs, want, wclock) in enumerate(_twins(rs, sched)):
        _same_rows(got, c, logs, f"sched {sched}")
        _same_state(st, c, want, f"sched {sched}", before)
        assert clock[0][c] == wclock[0][0] and clock[1][c] == wclock[1][0]
    assert (got["rbg_to_user"] >= 0).any()


def _against_the_oracle(rs, oracle, sched, r, g):
    grids = _grids(3, r)
    b, before = _batch(rs, sched, _configs(rs), r=r, g=g)
    got = b.run_logged(N_TTIS)
    st = b.state()
    b.close()
    for c, (ues, w, e, p) in enumerate(ROWS):
        n = NC[c]
        cell = oracle.Cell(list(ues), r, g, sched, weights=list(w), epsilon=list(e), psi=list(p))
        logs = cell.run_synth(np.ascontiguousarray(grids[c][:, :n]), int(SEEDS[c]), N_TTIS, phy_error_draws=0)
        ost = cell.state()
        np.testing.assert_array_equal(got["rbg_to_user"][c], logs["rbg_to_user"], err_msg=f"cell {c} RBG map")
        np.testing.assert_array_equal(got["tbs_bits"][c][:, :n], logs["tbs_bits"], err_msg=f"cell {c} TBS")
        assert not got["tbs_bits"][c][:, n:].any()
        np.testing.assert_array_equal(st["cum_bytes"][c, :n], ost["cum_bytes"])
        np.testing.assert_array_equal(st["cum_rbs"][c, :n], ost["cum_rbs"])
        assert st["avg_rate"][c, :n].tobytes() == ost["avg_rate"].tobytes(), f"cell {c} PF averages differ"
        assert st["slice_state"][c].tobytes() == ost["slice_state"].tobytes(), f"cell {c} slice state differs"
        for f in USER_STATE:
            assert st[f][c, n:].tobytes() == before[f][c, n:].tobytes(), f"cell {c}: {f} of an absent user was touched"


@pytest.mark.parametrize("sched", [9, 7])
def test_every_cell_is_the_oracle_of_its_users(rs, oracle, sched):
    _against_the_oracle(rs, oracle, sched, R, G)


def test_the_oracle_at_25_rbgs_of_4(rs, oracle):
    _against_the_oracle(rs, oracle, 9, 25, 4)


@pytest.mark.parametrize("sched", [9, 8, 7, 1])
def test_run_time_builds_serve_a_ragged_batch(rs, sched):
    """jit=True, selfcheck=1: the general build serves a logged launch, the lean build an unlogged one of 256 TTIs; both against the
    built-in twins of n_c users."""
    b, before = _batch(rs, sched, _configs(rs), jit=True, selfcheck=1)
    assert b.jit_status()[0] == 1, b.jit_status()
    got = b.run_logged(N_TTIS)
    assert b.jit_status()[0] == 1 and b.kernel_name == "rs_cell_kernel_jit", b.jit_status()
    st = b.state()
    b.close()
    for c, (logs, want, _) in enumerate(_twins(rs, sched)):
        _same_rows(got, c, logs, f"sched {sched}, general build")
        _same_state(st, c, want, f"sched {sched}, general build", before)
    n_long = 256
    b, before = _batch(rs, sched, _configs(rs), n_epochs=7, jit=True, selfcheck=1)
    b.run(n_long)
    status = b.jit_status()
    assert status[0] == 1 and "general and lean" in status[1], status
    st = b.state()
    b.close()
    for c, (_, want, _) in enumerate(_twins(rs, sched, n_long, logged=False)):
        _same_state(st, c, want, f"sched {sched}, lean build", before)


def test_scheduler_1_all_users_per_rbg_form(rs):
    """from 1 000 users on a run-time build of scheduler 1 ranks all users of an RBG on one wave and relies on zero reciprocals behind
    the last user: two cells of 1 024 and of 997 users (no multiple of 8) in a batch of 1 024, bait as above, against built-in twins"""
    big, small = rs.SliceConfig([256] * 4), rs.SliceConfig([256, 256, 256, 229])
    counts = (big.n_users, small.n_users)
    grids = synth_cqi(12, (2, 3, big.n_users, R), HIST)
    grids[1, :, small.n_users:, :] = 15
    b = rs.BatchScheduler(big, R, G, 2, sched=1, jit=True, selfcheck=1)
    b.set_cell_configs([big, small])
    b.seed(SEEDS[:2])
    b.upload_cqi_epochs(grids)
    avg = b.state()["avg_rate"]
    avg[1, small.n_users:] = BAIT_AVG
    b.write_state(avg_rate=avg)
    got, st = b.run_logged(N_TTIS), b.state()
    assert b.jit_status()[0] == 1 and b.kernel_name == "rs_cell_kernel_jit", b.jit_status()
    b.close()
    for c, (cfg, n) in enumerate(zip((big, small), counts)):
        t = rs.BatchScheduler(cfg, R, G, 1, sched=1)
        t.seed(SEEDS[c:c + 1])
        t.upload_cqi_epochs(np.ascontiguousarray(grids[c:c + 1, :, :n]))
        want, wst = t.run_logged(N_TTIS), t.state()
        t.close()
        np.testing.assert_array_equal(got["rbg_to_user"][c], want["rbg_to_user"][0], err_msg=f"cell {c}")
        np.testing.assert_array_equal(got["tbs_bits"][c][:, :n], want["tbs_bits"][0], err_msg=f"cell {c}")
        for f in USER_STATE:
            assert st[f][c, :n].tobytes() == wst[f][0].tobytes(), f"cell {c}, {f}"
    assert (st["avg_rate"][1, small.n_users:] == BAIT_AVG).all() and not st["cum_bytes"][1, small.n_users:].any()


def test_the_autotune_trials_carry_the_switch(rs):
    n_long = 256
    b, before = _batch(rs, 8, _configs(rs), n_epochs=7, jit=True, autotune=True, selfcheck=1)
    b.run(n_long)
    n, report = b.autotune_report()
    assert n >= 2 and "REJECTED" not in report and b.jit_status()[0] == 1, (report, b.jit_status())
    st = b.state()
    b.close()
    for c, (_, want, _) in enumerate(_twins(rs, 8, n_long, logged=False)):
        _same_state(st, c, want, "sched 8, autotuned lean build", before)


@pytest.mark.parametrize("sched", [9, 10])
def test_grant_records(rs, sched):
    b, before = _batch(rs, sched, _configs(rs))
    bound = b.grant_bound()
    recs = b.run_grant_records(N_TTIS)
    st = b.state()
    b.close()
    per_cell = [sum(min(n, R) for n in sizes) if sched == 10 else min(NC[c], R) for c, (sizes, _, _, _) in enumerate(ROWS)]
    assert bound == max(per_cell)
    for c, ((wbound, want_recs), want, _) in enumerate(_twins(rs, sched, records=True)):
        assert wbound == per_cell[c]
        assert len(recs[c]) == len(want_recs) and recs[c].tobytes() == want_recs.tobytes(), f"cell {c}"
        assert (recs[c]["user"] < NC[c]).all(), f"cell {c}: a record names an absent user"
        _same_state(st, c, want, f"sched {sched}, records launch", before)
    assert sum(len(x) for x in recs) > 0


def test_reducers_skip_the_absent_users(rs):
    cfgs = _configs(rs)
    b, _ = _batch(rs, 9, cfgs)
    b.run(N_TTIS)
    st, tot, by = b.state(), b.slice_totals(), b.slice_bytes()
    b.close()
    assert st["cum_bytes"][:, :1].sum() > 0
    for c in range(N_CELLS):
        m = cfgs[c].user_to_slice
        for f in ("cum_bytes", "cum_rbs"):
            want = np.array([st[f][c, :NC[c]][m == s].sum() for s in range(S)], np.int64)
            np.testing.assert_array_equal(tot[f][c], want, err_msg=f"cell {c} {f}")
    np.testing.assert_array_equal(by.astype(np.int64), tot["cum_bytes"].sum(axis=0))


def test_checkpoint(rs):
    cfgs = _configs(rs)
    whole, _ = _batch(rs, 9, cfgs)
    whole.run(120)
    want = whole.state()
    whole.close()
    first, _ = _batch(rs, 9, cfgs)
    first.run(60)
    blob = first.checkpoint()
    first.close()
    second, _ = _batch(rs, 9, cfgs, bait=False)
    second.restore(blob)
    second.run(60)
    got = second.state()
    second.close()
    for f in USER_STATE + ("slice_state",):
        assert got[f].tobytes() == want[f].tobytes(), f
    # other counts (row F with its last user present: the same slices but for the suffix), and uniform rows: refused
    other, _ = _batch(rs, 9, cfgs[:5] + [cfgs[0], cfgs[6]], bait=False)
    with pytest.raises(rs.RadioSaberError) as err:
        other.restore(blob)
    assert "configured differently" in str(err.value)
    other.close()
    flat, _ = _batch(rs, 9, [cfgs[0]] * N_CELLS, bait=False)
    with pytest.raises(rs.RadioSaberError):
        flat.restore(blob)
    flat.close()


def _refused(rs, b, code, *words, m=None):
    L = rs.lib()
    before = [b.cell_config(c) for c in range(N_CELLS)]
    users = b.cell_users()
    held = np.ascontiguousarray(m, np.int32)
    rc = L.rs_batch_set_cell_configs(b._h, None, None, None, held.ctypes.data_as(L.rs_batch_set_cell_configs.argtypes[4]))
    msg = L.rs_last_error().decode()
    assert rc == code, (rc, msg)
    for w in words:
        assert w in msg, msg
    after = [b.cell_config(c) for c in range(N_CELLS)]
    for x, y in zip(before, after):
        assert all(x[k].tobytes() == y[k].tobytes() for k in x), "a refused call changed a row"
    np.testing.assert_array_equal(b.cell_users(), users)


def test_refusals(rs):
    INVALID, STATE = -1, -4
    cfgs = _configs(rs)
    maps = rs.BatchScheduler.padded_maps(cfgs, U)
    for preset in (False, True):
        b = rs.BatchScheduler(_full(rs), R, G, N_CELLS, sched=9)
        if preset:
            b.set_cell_configs(cfgs)
        b.seed(SEEDS)
        b.upload_cqi_epochs(_grids(3))
        bad = maps.copy(); bad[2, 20] = -1
        _refused(rs, b, INVALID, "cell 2", "user 21", m=bad)          # an absent user in the middle: a slice id behind it
        bad = maps.copy(); bad[3, :] = -1
        _refused(rs, b, INVALID, "cell 3", "user 0", m=bad)           # a row of absent users alone
        bad = maps.copy(); bad[5, 95] = -2
        _refused(rs, b, INVALID, "cell 5", "user 95", m=bad)          # another negative value
        bad = maps.copy(); bad[4, 95] = S
        _refused(rs, b, INVALID, "cell 4", "user 95", m=bad)          # S stays out of range
        b.run(5)
        _refused(rs, b, STATE, "after TTIs", m=maps)
        b.close()
    # the shared configuration takes no absent user
    full = _full(rs)

    class LastUserAbsent(rs.SliceConfig):
        user_to_slice = property(lambda self: np.append(rs.SliceConfig.user_to_slice.fget(self)[:-1], -1).astype(np.int32))

    with pytest.raises(rs.RadioSaberError) as err:
        rs.BatchScheduler(LastUserAbsent(list(ROWS[0][0])), R, G, 1, sched=9)
    assert "user 95" in str(err.value) and "out of range" in str(err.value)
    # scheduler 11 and the queue model
    b = rs.BatchScheduler(full, R, G, N_CELLS, sched=11)
    _refused(rs, b, INVALID, "scheduler 11", m=maps)
    b.close()
    b = rs.BatchScheduler(full, R, G, N_CELLS, sched=9)
    b.set_bearers(full.bearer_kinds())
    _refused(rs, b, STATE, "queue model", m=maps)
    b.close()


def test_cell_users_with_and_without_rows(rs):
    b = rs.BatchScheduler(_full(rs), R, G, N_CELLS, sched=9)
    np.testing.assert_array_equal(b.cell_users(), [U] * N_CELLS)
    b.set_cell_configs([_configs(rs)[0]] * N_CELLS)
    np.testing.assert_array_equal(b.cell_users(), [U] * N_CELLS)
    b.set_cell_configs(_configs(rs))
    np.testing.assert_array_equal(b.cell_users(), NC)
    for c in range(N_CELLS):
        row = b.cell_config(c)["user_to_slice"]
        np.testing.assert_array_equal(row[:NC[c]], _configs(rs)[c].user_to_slice)
        assert (row[NC[c]:] == rs.api.RS_USER_ABSENT).all()
    b.close()


@pytest.mark.parametrize("sched", [9, 7, 1])
def test_rows_without_an_absent_user_run_as_before(rs, sched):
    """rows of 96 users each (tests/test_gpu_batch_cell_configs.py's shapes) take the code path they took: against one-cell twins"""
    sizes = [[24, 24, 24, 24], [70, 1, 0, 25], [7, 9, 33, 47], [96, 0, 0, 0], [24, 24, 24, 24], [48, 48, 0, 0], [1, 1, 1, 93]]
    cfgs = [rs.SliceConfig(s) for s in sizes]
    grids = _grids(3)
    b = rs.BatchScheduler(cfgs[0], R, G, N_CELLS, sched=sched)
    b.set_cell_configs(cfgs)
    b.seed(SEEDS)
    b.upload_cqi_epochs(grids)
    got, st = b.run_logged(N_TTIS), b.state()
    b.close()
    for c, cfg in enumerate(cfgs):
        t = rs.BatchScheduler(cfg, R, G, 1, sched=sched)
        t.seed(SEEDS[c:c + 1])
        t.upload_cqi_epochs(grids[c:c + 1])
        want, wst = t.run_logged(N_TTIS), t.state()
        t.close()
        for f in LOG_FIELDS:
            np.testing.assert_array_equal(got[f][c], want[f][0], err_msg=f"cell {c}, {f}")
        for f in USER_STATE + ("slice_state",):
            assert st[f][c].tobytes() == wst[f][0].tobytes(), f"cell {c}, {f}"


def _ref_config(sizes):
    return {"ues_per_slice": list(sizes), "slices": [dict(n_slices=1, weight=1.0 / len(sizes), algo_alpha=0, algo_beta=0, algo_epsilon=1, algo_psi=1)
                                                     for _ in sizes]}


def test_run_experiment_runs_configs_of_different_user_counts_as_one_batch(rs, tmp_path):
    """two configurations of 4 slices x {5, 12} users and two seeds through tools/run_experiment.py: four logs, each byte for byte the
    log of its single run"""
    tool = [sys.executable, str(ROOT / "tools" / "run_experiment.py"), "--sched", "9", "--duration", "0.12", "--nb-rbs", "12", "--rbg-size", "2"]
    names = {"ue5": [5] * 4, "ue12": [12] * 4}
    for name, sizes in names.items():
        (tmp_path / f"{name}.json").write_text(json.dumps(_ref_config(sizes)))
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
