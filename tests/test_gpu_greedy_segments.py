"""GPU parity for MaximizeCell's greedy scan over the array the introsort loop leaves (shape-specialised builds up to 32 RBGs:
no counting sort; rs_sort_device.h tags every record with its last sub-range, rs_interslice.h orders on wave 0 only the records
its vectors hold).  Every case runs the lean build (an unlogged launch) and the general build (a logged one) of one batch over
120 TTIs -- three CQI refreshes -- bitwise against the oracle; the shapes are the ones at which the first vector and the
compaction take another path.  tests/test_greedy_segments_model.py is the CPU model of the same steps."""
import json

import numpy as np
import pytest

from conftest import GOLDEN, synth_cqi
from test_greedy_segments_model import SHAPES, greedy_segments, loop  # noqa: F401  (loop: the fixture)

pytestmark = pytest.mark.gpu

HIST = (152600, 56656, 270880, 2088792, 3509504, 1595568, 4145392, 5295816, 1903424,
        6890232, 4770864, 2842552, 3579624, 96000, 1227696)
N_LEAN, N_LOGGED = 50, 70  # refreshes at TTI 40 (lean launch) and 80 (logged launch)


def _run(rs, oracle, monkeypatch, ues, R, G, grids, weights=None, slice_keys=False, extra=None):
    """grids [n_cells][3][U][R].  Returns (the logged launch's outputs, heap-sort counters) after full parity."""
    monkeypatch.setenv("RS_JIT_LEAN_MIN_TTIS", "1")
    if extra:
        monkeypatch.setenv("RS_JIT_EXTRA", extra)
    n_cells = grids.shape[0]
    S = len(ues)
    weights = weights or [1.0 / S] * S
    sc = rs.SliceConfig(ues, weight=weights)
    seeds = np.arange(n_cells, dtype=np.uint32) * 7919 + 805290992
    b = rs.BatchScheduler(sc, R, G, n_cells, sched=9, jit=True)
    assert b.kernel_name == "rs_cell_kernel_jit", b.jit_status()
    b.seed(seeds)
    b.upload_cqi_epochs(grids)
    b.prepare_launch(N_LEAN)
    b.run(N_LEAN)  # lean build
    got = b.run_logged(N_LOGGED, slice_keys=slice_keys)  # general build
    st, hs = b.state(), b.heap_sorts()
    b.close()
    for c in range(n_cells):
        cell = oracle.Cell(ues, R, G, 9, weights=weights)
        logs = cell.run_synth(grids[c], int(seeds[c]), N_LEAN + N_LOGGED)
        ost = cell.state()
        np.testing.assert_array_equal(got["rbg_to_user"][c], logs["rbg_to_user"][N_LEAN:], err_msg=f"cell {c} RBG map")
        np.testing.assert_array_equal(got["tbs_bits"][c], logs["tbs_bits"][N_LEAN:], err_msg=f"cell {c} TBS")
        np.testing.assert_array_equal(st["cum_bytes"][c], ost["cum_bytes"])
        np.testing.assert_array_equal(st["cum_rbs"][c], ost["cum_rbs"])
        assert st["avg_rate"][c].tobytes() == ost["avg_rate"].tobytes(), f"cell {c} PF averages differ"
        assert st["slice_state"][c].tobytes() == ost["slice_state"].tobytes(), f"cell {c} slice state differs"
    return got, hs


@pytest.mark.parametrize("ues,R,G", [([5] * 4, 16, 4),    # 64 records: the first vector is the whole array
                                     ([5] * 5, 13, 4)])   # 65 records: one record past the first vector
def test_arrays_of_one_vector_and_one_record_more(rs, oracle, monkeypatch, ues, R, G):
    grids = synth_cqi(7300 + R, (3, 3, sum(ues), R), HIST)
    _run(rs, oracle, monkeypatch, ues, R, G, grids)


@pytest.mark.parametrize("extra", [None, "-DRS_GREEDY_SORTED"])
def test_two_valued_grids_long_tie_runs(rs, oracle, monkeypatch, extra):
    """500 records of two CQI values: tie runs of hundreds of records, sub-ranges straddling position 64.  Once more with the
    counting sort switched back on (-DRS_GREEDY_SORTED): the two forms agree with the oracle, hence with each other."""
    ues, R, G = [5] * 20, 25, 4
    rng = np.random.default_rng(41)
    grids = rng.choice(np.array([7, 12], np.uint8), size=(3, 3, sum(ues), R), p=[0.7, 0.3]).astype(np.uint8)
    grids[2] = rng.choice(np.array([9, 10], np.uint8), size=grids[2].shape).astype(np.uint8)
    _run(rs, oracle, monkeypatch, ues, R, G, grids, extra=extra)


def test_more_than_a_vector_of_live_records_behind_the_first(rs, oracle, monkeypatch, loop):
    """1 024 records, four slices with nearly all the weight: the first vector grants a few RBGs and leaves more than 64 records
    live, so the survivors need several vectors, cut at sub-range starts.  The decision log's keys and quotas, put through the CPU
    model of the device's steps, say so."""
    ues, R, G = [2] * 32, 32, 4
    S = len(ues)
    weights = [0.22] * 4 + [0.12 / 28] * 28
    grids = synth_cqi(7411, (2, 3, sum(ues), R), HIST)
    got, _ = _run(rs, oracle, monkeypatch, ues, R, G, grids, weights=weights, slice_keys=True)
    assert SHAPES[R * S] == (R, S)
    ttis = range(0, N_LOGGED, 5)
    keys = [got["slice_cqi"][0, n].reshape(-1) for n in ttis]  # array index rbg * S + slice
    deep = 0
    for n, k, (ids, seg) in zip(ttis, keys, loop(keys)):
        arr = [(int(k[i]), int(i) // S, int(i) % S) for i in ids]
        stats = {}
        owner = greedy_segments(arr, seg, R, got["quota"][0, n].astype(np.int64), stats)
        users = np.array([got["slice_user"][0, n, r, owner[r]] if owner[r] >= 0 else -1 for r in range(R)])
        np.testing.assert_array_equal(got["rbg_to_user"][0, n], users, err_msg=f"TTI {n}: the model's grants")
        deep += stats.get("live_after_first", 0) > 64 and stats["vectors"] >= 3
    assert deep > 0, "no logged TTI left more than 64 live records behind its first vector"


@pytest.mark.parametrize("name", ["n500_wg", "n500_wg_long", "n500_wave"])
def test_heap_sorted_runs(rs, oracle, monkeypatch, name):
    """The sort-killer arrays as CQI grids, one UE per slice (tests/test_sort_killers.py): heap-sorted ranges -- runs of records
    that are each their own sub-range, longer than a vector in the workgroup-level arrays -- beside ordinary sub-ranges."""
    d = np.load(GOLDEN / "sort_killers.npz")
    meta = json.loads(bytes(d["meta"]).decode())
    assert name in meta
    R, G, S = 25, 4, 20
    k = np.ascontiguousarray(d[name].reshape(R, S).T, np.uint8)  # grid[u][r] = keys[r * S + u]
    rnd = synth_cqi(7500, (S, R), HIST)
    grids = np.stack([np.stack([k, rnd, k]), np.stack([rnd, k, rnd]), np.stack([k, k, k])])
    _, hs = _run(rs, oracle, monkeypatch, [1] * S, R, G, grids)
    # cell 2 sorts the killer in every TTI, cell 0 in 80 of 120, cell 1 in 40
    assert hs[2].sum() >= N_LEAN + N_LOGGED and hs[0].sum() >= 80 and hs[1].sum() >= 40, hs
