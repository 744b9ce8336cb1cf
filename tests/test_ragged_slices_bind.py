"""The shapes of tests/test_gpu_batch_ragged_slices.py bind (not gpu, oracle only): for every row with 1 < S_c < S and each of
schedulers 8, 9, 10, 101 and 103 the oracle of the true S_c differs, within the run, from the oracle of the same users with S - S_c
empty zero-weight slices behind them.  A device that ran such a cell as the padded one (the batch's S as the rotations' modulus or as
the sort's length) is then told apart from one that knows S_c.  Blind shapes exist -- rows of one present slice on every scheduler;
for 8, 10, 101, 103 shapes whose PRBs and RBGs divide without remainders (R = 6, G = 2 with three equal weights; R = 25, G = 4 with
five slices of 0.2) -- so this is checked, not assumed.

The rows live here; the GPU tests import them."""
import functools

import numpy as np
import pytest

from conftest import synth_cqi
from test_gpu_parity import HIST

SCHEDS_BIND = [8, 9, 10, 101, 103]

# shape A: S = 4, U = 96, R = 7, G = 3, 90 TTIs.  (sizes, weights, eps, psi)
A = dict(S=4, U=96, R=7, G=3, n_ttis=90)
ROWS_A = [
    ([24, 24, 24, 24], [0.25] * 4, [1] * 4, [1] * 4),
    ([24, 24, 24], [1 / 3] * 3, [1] * 3, [1] * 3),
    ([7, 9, 33], [0.5, 0.3, 0.2], [1] * 3, [1, 0, 1]),
    ([30, 20], [0.7, 0.3], [1] * 2, [1] * 2),          # N_c = 14 <= 16: the insertion sort alone
    ([40], [1.0], [1], [1]),                            # N_c = 7
    ([32, 32, 32], [1 / 3] * 3, [1] * 3, [1] * 3),      # fewer slices, all 96 users
]
# shape B: S = 20, R = 25, G = 4, 5 users per slice; shape C: S = 20, R = 64, G = 8, 5 users per slice
B = dict(S=20, U=100, R=25, G=4, n_ttis=90, counts=[13, 19, 20])
C_ = dict(S=20, U=100, R=64, G=8, n_ttis=45, counts=[5, 10, 15, 20])


def even_row(k, per=5):
    return ([per] * k, [1.0 / k] * k, [1] * k, [1] * k)


@functools.lru_cache(maxsize=None)
def grids(seed, n_cells, n_epochs, U, R):
    g = synth_cqi(seed, (n_cells, n_epochs, U, R), HIST)
    g.setflags(write=False)
    return g


def _differs(oracle, row, S, R, G, sched, n_ttis, grid, seed):
    ues, w, e, p = row
    k = S - len(ues)
    n = sum(ues)
    g = np.ascontiguousarray(grid[:, :n])
    true = oracle.Cell(list(ues), R, G, sched, weights=list(w), epsilon=list(e), psi=list(p))
    pad = oracle.Cell(list(ues) + [0] * k, R, G, sched, weights=list(w) + [0.0] * k, epsilon=list(e) + [1] * k, psi=list(p) + [1] * k)
    a = true.run_synth(g, seed, n_ttis, phy_error_draws=0)
    b = pad.run_synth(g, seed, n_ttis, phy_error_draws=0)
    return not (np.array_equal(a["rbg_to_user"], b["rbg_to_user"]) and np.array_equal(a["tbs_bits"], b["tbs_bits"]))


@pytest.mark.parametrize("sched", SCHEDS_BIND)
def test_shape_a_rows_bind(oracle, sched):
    g = grids(21, len(ROWS_A), 3, A["U"], A["R"])
    for c, row in enumerate(ROWS_A):
        if 1 < len(row[0]) < A["S"]:
            assert _differs(oracle, row, A["S"], A["R"], A["G"], sched, A["n_ttis"], g[c], 805290992 + 7919 * c), f"row {c} is blind for scheduler {sched}"


@pytest.mark.parametrize("sched", [8, 9, 10])
@pytest.mark.parametrize("shape", [B, C_], ids=["B", "C"])
def test_shapes_b_and_c_bind(oracle, sched, shape):
    g = grids(22 if shape is B else 23, len(shape["counts"]), (shape["n_ttis"] + 39) // 40, shape["U"], shape["R"])
    for c, k in enumerate(shape["counts"]):
        if k < shape["S"]:
            assert _differs(oracle, even_row(k), shape["S"], shape["R"], shape["G"], sched, shape["n_ttis"], g[c], 805290992 + 7919 * c), \
                f"{k} of {shape['S']} slices is blind for scheduler {sched}"
