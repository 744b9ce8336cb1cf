"""Cells of different slice counts in one batch (gpu): rs_batch_set_cell_configs_n gives every cell a slice count S_c <= S, and cell c
then runs, to the bit, like a one-cell batch created with S_c slices (and n_c users) from the heads of its rows, while the absent
slices behind them take part in nothing and their slice_state words are never written.

Shapes and rows are tests/test_ragged_slices_bind.py's, which shows on the oracle that each of them tells S_c from a padding with
empty zero-weight slices:
  A  S = 4, U = 96, R = 7, G = 3, 90 logged TTIs: rows of 4, 3, 3, 2, 1 and 3 slices (N_c = 28, 21, 21, 14, 7, 21 records: at and
     below the sort's 16-element threshold too), the last with all 96 users; every scheduler, built-in kernels and run-time builds
  B  S = 20, R = 25, G = 4: cells of 13, 19 and 20 slices -- the vector scan, held winners and the tagged sort of run-time builds
  C  S = 20, R = 64, G = 8, 512 threads: cells of 5, 10, 15 and 20 slices -- N_c = 320 ... 1 280 records under three position slots
     per thread, whole slots empty
and a depth-limit cell: 20 of 24 slices on a grid that sends std::sort into its heap-sort fallback at 500 records.
The bait: an absent slice's slice_state holds a recognisable double outside rs_batch_write_state's domain rule; absent users as in
tests/test_gpu_batch_ragged_cells.py (CQI 15 everywhere, an average next to the clamp, recognisable counters).
The twins (one-cell batches of S_c slices and n_c users on the built-in kernels) are run once per (shape, scheduler, length)."""
import functools
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from test_ragged_slices_bind import A, B, C_, ROWS_A, even_row, grids as _plain_grids
from test_sort_killers import _grid_maxcell

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
SCHEDS = [1, 7, 8, 9, 10, 101, 103]
TRANSPORT = (8, 9, 10, 101, 103)
LOG_FIELDS = ("rbg_to_user", "tbs_bits", "quota", "target", "nprb", "final_cqi", "mcs")
USER_LOG_FIELDS = ("tbs_bits", "nprb", "final_cqi", "mcs")   # [cells][TTIs][U]
SLICE_LOG_FIELDS = ("quota", "target")                       # [cells][TTIs][S]
USER_STATE = ("avg_rate", "cum_bytes", "cum_rbs")
BAIT_AVG, BAIT_BYTES, BAIT_RBS = 1.25, 0x0123456789ABCDE, 0x0FEDCBA98765
BAIT_SLICE = 1.0e9 + 0.125   # far outside the domain rule (5 nb_rbs (1 + sum |w|) + sum |offset| < 2^15), and >= 0 for NVS


class Shape:
    def __init__(self, name, dims, rows, grid_seed):
        self.name, self.rows = name, rows
        self.S, self.U, self.R, self.G, self.n_ttis = dims["S"], dims["U"], dims["R"], dims["G"], dims["n_ttis"]
        self.n_cells = len(rows)
        self.ns = [len(r[0]) for r in rows]
        self.nc = [sum(r[0]) for r in rows]
        self.seeds = np.arange(self.n_cells, dtype=np.uint32) * 7919 + 805290992
        self.grid_seed = grid_seed

    def configs(self, rs):
        return [rs.SliceConfig(list(ues), weight=list(w), algo_epsilon=list(e), algo_psi=list(p)) for ues, w, e, p in self.rows]

    def shared(self, rs):
        """the batch's own configuration: the (first) row of S slices and U users"""
        return next(cfg for cfg in self.configs(rs) if cfg.n_slices == self.S and cfg.n_users == self.U)

    @functools.lru_cache(maxsize=None)
    def grids(self, n_epochs):
        g = _plain_grids(self.grid_seed, self.n_cells, n_epochs, self.U, self.R).copy()
        for c, n in enumerate(self.nc):
            g[c, :, n:, :] = 15   # the bait
        g.setflags(write=False)
        return g


SHAPE_A = Shape("A", A, ROWS_A, 21)
SHAPE_B = Shape("B", B, [even_row(k) for k in B["counts"]], 22)
SHAPE_C = Shape("C", C_, [even_row(k) for k in C_["counts"]], 23)


def _bait(b, sh):
    """absent users' averages and absent slices' state words through write_state, the users' counters through a checkpoint of the batch
    itself (no TTI run yet); returns the baited state"""
    st = b.state()
    for c in range(sh.n_cells):
        st["avg_rate"][c, sh.nc[c]:] = BAIT_AVG
        st["slice_state"][c, sh.ns[c]:] = BAIT_SLICE + np.arange(sh.S - sh.ns[c])
    avg = st["avg_rate"].copy()
    b.write_state(avg_rate=avg, slice_state=st["slice_state"].copy())
    if min(sh.nc) < sh.U:
        blob = bytearray(b.checkpoint())
        marker = np.ascontiguousarray(avg, np.float64).tobytes()
        off = bytes(blob).find(marker)
        assert off > 0 and bytes(blob).find(marker, off + 1) < 0
        n = sh.n_cells * sh.U
        off_cumb = off + (8 + 4) * n
        cumb = np.zeros((sh.n_cells, sh.U), np.int64)
        cumr = np.zeros((sh.n_cells, sh.U), np.int64)
        for c, k in enumerate(sh.nc):
            cumb[c, k:] = BAIT_BYTES + np.arange(sh.U - k)
            cumr[c, k:] = BAIT_RBS + np.arange(sh.U - k)
        blob[off_cumb:off_cumb + 8 * n] = cumb.tobytes()
        blob[off_cumb + 8 * n:off_cumb + 16 * n] = cumr.tobytes()
        b.restore(bytes(blob))
    got = b.state()
    for c in range(sh.n_cells):
        assert (got["slice_state"][c, sh.ns[c]:] == BAIT_SLICE + np.arange(sh.S - sh.ns[c])).all()
    return got


def _batch(rs, sh, sched, n_epochs=None, bait=True, configs=None, **kw):
    b = rs.BatchScheduler(sh.shared(rs), sh.R, sh.G, sh.n_cells, sched=sched, **kw)
    b.set_cell_configs(sh.configs(rs) if configs is None else configs)
    b.seed(sh.seeds)
    b.upload_cqi_epochs(sh.grids(n_epochs or (sh.n_ttis + 39) // 40))
    return (b, _bait(b, sh)) if bait else (b, None)


_TWINS = {}


def _twins(rs, sh, sched, n_ttis=None, logged=True, records=False):
    """one-cell batches of S_c slices and n_c users on the built-in kernels, one per row:
    [(rows / records / None, state, clock, heap sorts)], computed once"""
    n_ttis = n_ttis or sh.n_ttis
    key = (sh.name, sched, n_ttis, logged, records)
    if key not in _TWINS:
        out = []
        n_epochs = (n_ttis + 39) // 40
        for c, cfg in enumerate(sh.configs(rs)):
            b = rs.BatchScheduler(cfg, sh.R, sh.G, 1, sched=sched)
            b.seed(sh.seeds[c:c + 1])
            b.upload_cqi_epochs(np.ascontiguousarray(sh.grids(n_epochs)[c:c + 1, :, :sh.nc[c]]))
            if records:
                logs = (b.grant_bound(), b.run_grant_records(n_ttis)[0].copy())
            else:
                logs = b.run_logged(n_ttis, slice_keys=sched in TRANSPORT) if logged else b.run(n_ttis)
            out.append((logs, b.state(), b.clock(), int(b.heap_sorts().sum())))
            b.close()
        _TWINS[key] = out
    return _TWINS[key]


def _same_state(sh, st, c, want, what, before):
    n, k = sh.nc[c], sh.ns[c]
    for f in USER_STATE:
        assert st[f][c, :n].tobytes() == want[f][0].tobytes(), f"{what}: cell {c}, {f} differs from the one-cell batch of its {k} slices"
        assert st[f][c, n:].tobytes() == before[f][c, n:].tobytes(), f"{what}: cell {c}, {f} of an absent user was touched"
    assert st["slice_state"][c, :k].tobytes() == want["slice_state"][0].tobytes(), f"{what}: cell {c}, slice state"
    assert st["slice_state"][c, k:].tobytes() == before["slice_state"][c, k:].tobytes(), f"{what}: cell {c}: an absent slice's state word was written"


def _same_rows(sh, got, c, want, what):
    n, k = sh.nc[c], sh.ns[c]
    for f in LOG_FIELDS:
        if f in USER_LOG_FIELDS:
            np.testing.assert_array_equal(got[f][c][:, :n], want[f][0], err_msg=f"{what}: cell {c}, {f}")
            assert not got[f][c][:, n:].any(), f"{what}: cell {c}, {f}: an absent user's row is not an unserved user's"
        elif f in SLICE_LOG_FIELDS:
            np.testing.assert_array_equal(got[f][c][:, :k], want[f][0], err_msg=f"{what}: cell {c}, {f}")
            assert not got[f][c][:, k:].any(), f"{what}: cell {c}, {f}: an absent slice's entry is not 0"
        else:
            np.testing.assert_array_equal(got[f][c], want[f][0], err_msg=f"{what}: cell {c}, {f}")
    assert (got["rbg_to_user"][c] < n).all(), f"{what}: cell {c}: an RBG went to an absent user"
    if "slice_cqi" in got:
        np.testing.assert_array_equal(got["slice_cqi"][c][:, :, :k], want["slice_cqi"][0], err_msg=f"{what}: cell {c}, slice keys")
        np.testing.assert_array_equal(got["slice_user"][c][:, :, :k], want["slice_user"][0], err_msg=f"{what}: cell {c}, slice winners")
        assert not got["slice_cqi"][c][:, :, k:].any() and (got["slice_user"][c][:, :, k:] == -1).all(), f"{what}: cell {c}: keys of an absent slice"


def _against_the_oracle(sh, oracle, sched, got, st, what):
    grids = sh.grids((sh.n_ttis + 39) // 40)
    for c, (ues, w, e, p) in enumerate(sh.rows):
        n, k = sh.nc[c], sh.ns[c]
        cell = oracle.Cell(list(ues), sh.R, sh.G, sched, weights=list(w), epsilon=list(e), psi=list(p))
        logs = cell.run_synth(np.ascontiguousarray(grids[c][:, :n]), int(sh.seeds[c]), sh.n_ttis, phy_error_draws=0)
        ost = cell.state()
        np.testing.assert_array_equal(got["rbg_to_user"][c], logs["rbg_to_user"], err_msg=f"{what}: cell {c} RBG map against the oracle")
        np.testing.assert_array_equal(got["tbs_bits"][c][:, :n], logs["tbs_bits"], err_msg=f"{what}: cell {c} TBS against the oracle")
        np.testing.assert_array_equal(st["cum_bytes"][c, :n], ost["cum_bytes"])
        np.testing.assert_array_equal(st["cum_rbs"][c, :n], ost["cum_rbs"])
        assert st["avg_rate"][c, :n].tobytes() == ost["avg_rate"].tobytes(), f"{what}: cell {c} PF averages differ from the oracle's"
        assert st["slice_state"][c, :k].tobytes() == ost["slice_state"].tobytes(), f"{what}: cell {c} slice state differs from the oracle's"


def _logged_against_twins_and_oracle(rs, oracle, sh, sched, what, with_oracle=True, **kw):
    b, before = _batch(rs, sh, sched, **kw)
    np.testing.assert_array_equal(b.cell_slices(), sh.ns)
    np.testing.assert_array_equal(b.cell_users(), sh.nc)
    got = b.run_logged(sh.n_ttis, slice_keys=sched in TRANSPORT)
    if kw.get("jit"):
        assert b.jit_status()[0] == 1 and b.kernel_name == "rs_cell_kernel_jit", b.jit_status()
    st, clock, heaps = b.state(), b.clock(), b.heap_sorts().sum(axis=1)
    b.close()
    for c, (logs, want, wclock, wheaps) in enumerate(_twins(rs, sh, sched)):
        _same_rows(sh, got, c, logs, what)
        _same_state(sh, st, c, want, what, before)
        assert clock[0][c] == wclock[0][0] and clock[1][c] == wclock[1][0], f"{what}: cell {c} clock"
        if not kw.get("jit"):   # (a run-time build's self-check launches count too)
            assert heaps[c] == wheaps, f"{what}: cell {c} took {heaps[c]} heap sorts, its one-cell batch {wheaps}"
    assert (got["rbg_to_user"] >= 0).any()
    if with_oracle:
        _against_the_oracle(sh, oracle, sched, got, st, what)


# ---------------- shape A ----------------
@pytest.mark.parametrize("jit", [False, True], ids=["builtin", "jit"])
@pytest.mark.parametrize("sched", SCHEDS)
def test_shape_a_every_cell_is_the_one_cell_batch_of_its_slices(rs, oracle, sched, jit):
    kw = dict(jit=True, selfcheck=1) if jit else {}
    _logged_against_twins_and_oracle(rs, oracle, SHAPE_A, sched, f"shape A, sched {sched}, {'run-time build' if jit else 'built-in'}", with_oracle=not jit, **kw)


# ---------------- shape B: vector scan, held winners, the tagged sort ----------------
@pytest.mark.parametrize("sched", [8, 9, 10])
def test_shape_b_run_time_builds(rs, oracle, sched):
    sh = SHAPE_B
    _logged_against_twins_and_oracle(rs, oracle, sh, sched, f"shape B, sched {sched}, general build", jit=True, selfcheck=1)
    n_long = 256
    b, before = _batch(rs, sh, sched, n_epochs=7, jit=True, selfcheck=1)
    b.run(n_long)
    status = b.jit_status()
    assert status[0] == 1 and "general and lean" in status[1], status
    st = b.state()
    b.close()
    for c, (_, want, _, _) in enumerate(_twins(rs, sh, sched, n_long, logged=False)):
        _same_state(sh, st, c, want, f"shape B, sched {sched}, lean build", before)


@pytest.mark.parametrize("sched", [9, 10])
def test_shape_b_grant_records(rs, sched):
    sh = SHAPE_B
    b, before = _batch(rs, sh, sched, jit=True, selfcheck=1)
    bound = b.grant_bound()
    recs = b.run_grant_records(sh.n_ttis)
    st = b.state()
    b.close()
    per_cell = [sum(min(n, sh.R) for n in sizes) if sched == 10 else min(sh.nc[c], sh.R) for c, (sizes, _, _, _) in enumerate(sh.rows)]
    assert bound == max(per_cell)
    for c, ((wbound, want_recs), want, _, _) in enumerate(_twins(rs, sh, sched, records=True)):
        assert wbound == per_cell[c]
        assert len(recs[c]) == len(want_recs) and recs[c].tobytes() == want_recs.tobytes(), f"cell {c}"
        assert (recs[c]["user"] < sh.nc[c]).all(), f"cell {c}: a record names an absent user"
        _same_state(sh, st, c, want, f"shape B, sched {sched}, records launch", before)
    assert sum(len(x) for x in recs) > 0


# ---------------- shape C: as shipped, three position slots per thread, whole slots empty ----------------
@pytest.mark.parametrize("jit", [False, True], ids=["builtin", "jit"])
@pytest.mark.parametrize("sched", [8, 9, 10])
def test_shape_c_512_threads(rs, oracle, sched, jit):
    kw = dict(jit=True, selfcheck=1) if jit else {}
    _logged_against_twins_and_oracle(rs, oracle, SHAPE_C, sched, f"shape C, sched {sched}, {'run-time build' if jit else 'built-in'}", with_oracle=sched == 9 and not jit,
                                     threads_per_cell=512, **kw)


# ---------------- the depth limit is N_c's ----------------
@pytest.mark.parametrize("jit", [False, True], ids=["builtin", "jit"])
def test_the_depth_limit_is_the_cells_own(rs, oracle, jit):
    """S = 24, R = 25, G = 4, one user per slice.  Cell 0: 20 slices on sort_killers.npz's n500_wg grid (500 records: the array on which
    libstdc++'s introsort runs out of 2 * floor(log2 500) levels) and four absent users; cell 1: all 24 slices on random grids.  Cell 0
    is oracle.Cell([1] * 20, ...), and its heap-sort count is at least its killer TTIs."""
    S, R, G, n_ttis = 24, 25, 4, 30
    keys = np.load(ROOT / "tests" / "golden" / "sort_killers.npz")["n500_wg"]
    grid0 = np.concatenate([_grid_maxcell(keys, R, 20), np.full((4, R), 15, np.uint8)])
    g = np.stack([grid0, _plain_grids(24, 1, 1, S, R)[0, 0]])[:, None]      # [cell][epoch][U][R]
    seeds = np.array([3, 5], np.uint32)
    small, full = rs.SliceConfig([1] * 20), rs.SliceConfig([1] * S)
    b = rs.BatchScheduler(full, R, G, 2, sched=9, **(dict(jit=True, selfcheck=1) if jit else {}))
    b.set_cell_configs([small, full])
    b.seed(seeds)
    b.upload_cqi_epochs(g)
    st0 = b.state()
    st0["slice_state"][0, 20:] = BAIT_SLICE
    b.write_state(slice_state=st0["slice_state"])
    got, st, heaps = b.run_logged(n_ttis), b.state(), b.heap_sorts().sum(axis=1)
    b.close()
    for c, (ues, n) in enumerate((([1] * 20, 20), ([1] * S, S))):
        cell = oracle.Cell(ues, R, G, 9)
        logs = cell.run_synth(np.ascontiguousarray(g[c][:, :n]), int(seeds[c]), n_ttis, phy_error_draws=0)
        np.testing.assert_array_equal(got["rbg_to_user"][c], logs["rbg_to_user"], err_msg=f"cell {c} RBG map")
        np.testing.assert_array_equal(got["tbs_bits"][c][:, :n], logs["tbs_bits"], err_msg=f"cell {c} TBS")
        assert st["slice_state"][c, :n].tobytes() == cell.state()["slice_state"].tobytes()
    assert (st["slice_state"][0, 20:] == BAIT_SLICE).all()
    assert heaps[0] >= n_ttis, f"the heap-sort fallback ran {heaps[0]} times in {n_ttis} killer TTIs"


# ---------------- host side ----------------
def test_checkpoint_and_resume(rs):
    sh = SHAPE_A
    whole, _ = _batch(rs, sh, 9, n_epochs=3)
    whole.run(120)
    want = whole.state()
    whole.close()
    first, _ = _batch(rs, sh, 9, n_epochs=3)
    first.run(60)
    blob = first.checkpoint()
    first.close()
    second, _ = _batch(rs, sh, 9, n_epochs=3, bait=False)
    second.restore(blob)
    second.run(60)
    got = second.state()
    second.close()
    for f in USER_STATE + ("slice_state",):
        assert got[f].tobytes() == want[f].tobytes(), f
    # other counts with the same rows (row [32, 32, 32] as three of four slices, the fourth empty): refused
    cfgs = sh.configs(rs)
    padded = rs.SliceConfig([32, 32, 32, 0], weight=[1 / 3] * 3 + [0.0], algo_epsilon=[1] * 4, algo_psi=[1] * 4)
    other, _ = _batch(rs, sh, 9, n_epochs=3, bait=False, configs=cfgs[:5] + [padded])
    np.testing.assert_array_equal(other.cell_slices(), sh.ns[:5] + [4])
    assert all(other.cell_config(5)[k].tobytes() == second_row.tobytes() for k, second_row in _row_of(rs, sh, 5).items()), \
        "the two batches differ in more than the count"
    with pytest.raises(rs.RadioSaberError) as err:
        other.restore(blob)
    assert "configured differently" in str(err.value)
    other.close()


def _row_of(rs, sh, c):
    b = rs.BatchScheduler(sh.shared(rs), sh.R, sh.G, sh.n_cells, sched=9)
    b.set_cell_configs(sh.configs(rs))
    row = b.cell_config(c)
    b.close()
    return row


def _call_n(rs, b, counts, w=None, e=None, p=None, m=None):
    L = rs.lib()
    t = L.rs_batch_set_cell_configs_n.argtypes
    arr = [None if x is None else np.ascontiguousarray(x, d) for x, d in ((counts, np.int32), (w, np.float64), (e, np.int32), (p, np.int32), (m, np.int32))]
    rc = L.rs_batch_set_cell_configs_n(b._h, *[None if a is None else a.ctypes.data_as(t[i + 1]) for i, a in enumerate(arr)])
    return rc, L.rs_last_error().decode()


def _refused(rs, b, code, *words, **args):
    n = b.n_cells
    before = [b.cell_config(c) for c in range(n)]
    counts, users = b.cell_slices(), b.cell_users()
    rc, msg = _call_n(rs, b, **args)
    assert rc == code, (rc, msg)
    for w in words:
        assert w in msg, msg
    for x, y in zip(before, [b.cell_config(c) for c in range(n)]):
        assert all(x[k].tobytes() == y[k].tobytes() for k in x), "a refused call changed a row"
    np.testing.assert_array_equal(b.cell_slices(), counts)
    np.testing.assert_array_equal(b.cell_users(), users)


def test_validation_names_cell_and_index(rs):
    INVALID, STATE = -1, -4
    sh = SHAPE_A
    cfgs = sh.configs(rs)
    maps = rs.BatchScheduler.padded_maps(cfgs, sh.U)
    ns = np.array(sh.ns, np.int32)
    for preset in (False, True):
        b = rs.BatchScheduler(sh.shared(rs), sh.R, sh.G, sh.n_cells, sched=9)
        if preset:
            b.set_cell_configs(cfgs)
        b.seed(sh.seeds)
        b.upload_cqi_epochs(sh.grids(3))
        bad = ns.copy(); bad[2] = 0
        _refused(rs, b, INVALID, "cell 2", "cell_slices[2] = 0", counts=bad, m=maps)
        bad = ns.copy(); bad[4] = sh.S + 1
        _refused(rs, b, INVALID, "cell 4", f"cell_slices[4] = {sh.S + 1}", counts=bad, m=maps)
        bad = maps.copy(); bad[3, 49] = 2                                      # row [30, 20]: slice 2 is absent
        _refused(rs, b, INVALID, "cell 3", "user 49", "slice 2", counts=ns, m=bad)
        bad = maps.copy(); bad[1, 71] = 3                                      # ... in front of the absent-user suffix
        _refused(rs, b, INVALID, "cell 1", "user 71", "slice 3", counts=ns, m=bad)
        w = np.full((sh.n_cells, sh.S), 0.25); w[2, 1] = np.nan                # a head entry: checked
        _refused(rs, b, INVALID, "cell 2", "slice_weight[1]", counts=ns, w=w, m=maps)
        e = np.ones((sh.n_cells, sh.S), np.int32); e[3, 1] = 2
        _refused(rs, b, INVALID, "cell 3", "slice 1", counts=ns, e=e, m=maps)
        # entries of absent slices: stored, returned as given, not validated
        w = np.full((sh.n_cells, sh.S), 0.25); w[4, 1:] = np.nan
        e = np.ones((sh.n_cells, sh.S), np.int32); e[4, 2] = 77
        p = np.ones((sh.n_cells, sh.S), np.int32); p[3, 3] = -5
        rc, msg = _call_n(rs, b, counts=ns, w=w, e=e, p=p, m=maps)
        assert rc == 0, msg
        row = b.cell_config(4)
        assert np.isnan(row["weight"][1:]).all() and row["algo_epsilon"][2] == 77 and b.cell_config(3)["algo_psi"][3] == -5
        np.testing.assert_array_equal(b.cell_slices(), ns)
        # write_state: an absent slice's word is outside the domain rule, a present slice's is not
        st = b.state()["slice_state"]
        st[4, 1:] = BAIT_SLICE
        b.write_state(slice_state=st)
        st[4, 0] = BAIT_SLICE
        with pytest.raises(rs.RadioSaberError) as err:
            b.write_state(slice_state=st)
        assert "cell 4" in str(err.value)
        b.run(5)
        _refused(rs, b, STATE, "after TTIs", counts=ns, m=maps)
        b.close()
    b = rs.BatchScheduler(sh.shared(rs), sh.R, sh.G, sh.n_cells, sched=11)
    _refused(rs, b, INVALID, "scheduler 11", counts=ns, m=maps)
    b.close()
    b = rs.BatchScheduler(sh.shared(rs), sh.R, sh.G, sh.n_cells, sched=9)
    b.set_bearers(sh.shared(rs).bearer_kinds())
    _refused(rs, b, STATE, "queue model", counts=ns, m=maps)
    b.close()
    b = rs.BatchScheduler(sh.shared(rs), sh.R, sh.G, sh.n_cells, sched=9)
    b.set_cell_configs(cfgs)
    with pytest.raises(rs.RadioSaberError):
        b.set_bearers(sh.shared(rs).bearer_kinds())
    b.close()


def test_null_counts_are_set_cell_configs_and_a_later_call_replaces(rs):
    sh = SHAPE_A
    full = [rs.SliceConfig(s) for s in ([24, 24, 24, 24], [70, 1, 0, 25], [7, 9, 33, 47], [96, 0, 0, 0], [24, 24, 24, 24], [48, 48, 0, 0])]
    maps = rs.BatchScheduler.padded_maps(full, sh.U)
    out = []
    for via_n in (False, True):
        b = rs.BatchScheduler(sh.shared(rs), sh.R, sh.G, sh.n_cells, sched=9)
        np.testing.assert_array_equal(b.cell_slices(), [sh.S] * sh.n_cells)      # a batch without rows
        if via_n:
            b.set_cell_configs(sh.configs(rs))                                    # ... replaced by the call below
            np.testing.assert_array_equal(b.cell_slices(), sh.ns)
            rc, msg = _call_n(rs, b, None, m=maps)
            assert rc == 0, msg
        else:
            b.set_cell_configs(full)
        np.testing.assert_array_equal(b.cell_slices(), [sh.S] * sh.n_cells)
        b.seed(sh.seeds)
        b.upload_cqi_epochs(sh.grids(3))
        got = b.run_logged(sh.n_ttis)
        out.append((got, b.state(), b.checkpoint()))
        b.close()
    for f in LOG_FIELDS:
        np.testing.assert_array_equal(out[0][0][f], out[1][0][f], err_msg=f)
    for f in USER_STATE + ("slice_state",):
        assert out[0][1][f].tobytes() == out[1][1][f].tobytes(), f
    # the configuration hash is the same: a checkpoint of the one loads into the other
    b = rs.BatchScheduler(sh.shared(rs), sh.R, sh.G, sh.n_cells, sched=9)
    rc, msg = _call_n(rs, b, None, m=maps)
    assert rc == 0, msg
    b.upload_cqi_epochs(sh.grids(3))
    b.restore(out[0][2])
    assert b.state()["avg_rate"].tobytes() == out[0][1]["avg_rate"].tobytes()
    b.close()


def test_upperbound_grant_bound_sums_over_each_cells_own_slices(rs):
    sh = SHAPE_A
    b, _ = _batch(rs, sh, 10, bait=False)
    assert b.grant_bound() == max(sum(min(n, sh.R) for n in sizes) for sizes, _, _, _ in sh.rows)
    b.close()
    b, _ = _batch(rs, sh, 9, bait=False)
    assert b.grant_bound() == min(max(sh.nc), sh.R)
    b.close()


def test_slice_totals_and_slice_bytes(rs):
    sh = SHAPE_A
    cfgs = sh.configs(rs)
    b, _ = _batch(rs, sh, 9)
    b.run(sh.n_ttis)
    st, tot, by = b.state(), b.slice_totals(), b.slice_bytes()
    b.close()
    assert st["cum_bytes"][:, :1].sum() > 0
    for c in range(sh.n_cells):
        m = cfgs[c].user_to_slice
        for f in ("cum_bytes", "cum_rbs"):
            want = np.array([st[f][c, :sh.nc[c]][m == s].sum() for s in range(sh.S)], np.int64)
            np.testing.assert_array_equal(tot[f][c], want, err_msg=f"cell {c} {f}")
            assert not tot[f][c, sh.ns[c]:].any(), f"cell {c}: {f} of an absent slice"
    np.testing.assert_array_equal(by.astype(np.int64), tot["cum_bytes"].sum(axis=0))


def _ref_config(sizes):
    return {"ues_per_slice": list(sizes), "slices": [dict(n_slices=1, weight=1.0 / len(sizes), algo_alpha=0, algo_beta=0, algo_epsilon=1, algo_psi=1)
                                                     for _ in sizes]}


def test_run_experiment_runs_configs_of_different_slice_counts_as_one_batch(rs, tmp_path):
    """four configurations of 1 to 4 slices (and different user counts) and two seeds through tools/run_experiment.py: eight logs, each
    byte for byte the log of its single run"""
    tool = [sys.executable, str(ROOT / "tools" / "run_experiment.py"), "--sched", "9", "--duration", "0.12", "--nb-rbs", "21", "--rbg-size", "3"]
    names = {"s1": [9], "s2": [5, 7], "s3": [4, 4, 4], "s4": [3, 3, 3, 2]}
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
    assert len(logs) == 8
