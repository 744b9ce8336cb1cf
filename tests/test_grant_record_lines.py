"""Grant records and the log (not gpu): logfmt.grant_record_lines writes from a cell's grant records, byte for byte, the lines
logfmt.stderr_lines writes from the dense rows of the same run; logfmt.grant_records_from_rows and rows_from_grant_records are each
other's inverse.  The rows are oracle runs (Cell.run_synth, 45 TTIs) of the shapes the GPU suite runs."""
import numpy as np
import pytest

from conftest import synth_cqi
from radiosaber_amd import logfmt

HIST = (152600, 56656, 270880, 2088792, 3509504, 1595568, 4145392, 5295816, 1903424,
        6890232, 4770864, 2842552, 3579624, 96000, 1227696)
SEED, N_TTIS = 805290992, 45
CASES = [(9, [5, 4, 3], 8, 2), (9, [5] * 20, 25, 4), (9, [4, 4, 4], 64, 8), (8, [5] * 20, 25, 4), (7, [5] * 20, 25, 4), (1, [5] * 20, 25, 4)]


def _rows(oracle, sched, ues, R, G):
    U = sum(ues)
    grids = synth_cqi(1, (2, U, R), HIST)
    cell = oracle.Cell(ues, R, G, sched)
    logs = cell.run_synth(grids, SEED, N_TTIS)
    m, tbs = logs["rbg_to_user"], logs["tbs_bits"]
    nprb = np.stack([np.bincount(row[row >= 0], minlength=U) * G for row in m]).astype(np.int32)
    uinfo = np.where(tbs // 8 > 0, nprb | (7 << 16) | (12 << 24), 0).astype(np.int32)   # (any final CQI / MCS: the lines do not print them)
    return cell, m, tbs, uinfo


@pytest.mark.parametrize("sched,ues,R,G", CASES)
def test_lines_from_records_are_the_lines_from_rows(oracle, sched, ues, R, G):
    cell, m, tbs, uinfo = _rows(oracle, sched, ues, R, G)
    U = sum(ues)
    recs = logfmt.grant_records_from_rows(tbs, uinfo, m)
    assert recs.dtype.itemsize == 32 and len(recs) == int((tbs // 8 > 0).sum()) > N_TTIS
    assert (np.diff(recs["tti"]) >= 0).all() and (recs["bytes"] > 0).all() and not recs["reserved"].any()
    rng = np.random.default_rng(3)
    starts = [(None, None), (rng.integers(0, 2**40, U), rng.integers(0, 2**33, U))]
    for cb0, cr0 in starts:
        for pf in (False, True):
            want = logfmt.stderr_lines(tbs, m, cell.u2s, G, first_ts=100, cum_bytes0=cb0, cum_rbs0=cr0, pf_format=pf)
            got = logfmt.grant_record_lines(recs, cell.u2s, first_ts=100, cum_bytes0=cb0, cum_rbs0=cr0, pf_format=pf)
            assert got == want and len(want) == len(recs)
    # two launches, 7 + 38 TTIs: the records' TTI numbers go on counting, the counters carry over
    first = recs[recs["tti"] < 7]
    lines = logfmt.grant_record_lines(first, cell.u2s)
    cb = np.bincount(first["user"], weights=first["bytes"], minlength=U).astype(np.int64)
    cr = np.bincount(first["user"], weights=first["nprb"], minlength=U).astype(np.int64)
    lines += logfmt.grant_record_lines(recs[recs["tti"] >= 7], cell.u2s, cum_bytes0=cb, cum_rbs0=cr)
    assert lines == logfmt.stderr_lines(tbs, m, cell.u2s, G)
    assert lines[-1] == logfmt.stderr_lines(tbs[7:], m[7:], cell.u2s, G, first_ts=107, cum_bytes0=cb, cum_rbs0=cr)[-1]


@pytest.mark.parametrize("sched,ues,R,G", CASES)
def test_rows_from_records_invert_records_from_rows(oracle, sched, ues, R, G):
    _, m, tbs, uinfo = _rows(oracle, sched, ues, R, G)
    U = sum(ues)
    recs = logfmt.grant_records_from_rows(tbs, uinfo, m, first_tti=300)
    assert recs["tti"].min() >= 300
    rows = logfmt.rows_from_grant_records(recs, N_TTIS, U, R, 300)
    np.testing.assert_array_equal(rows["tbs_bits"], tbs)
    np.testing.assert_array_equal(rows["uinfo"], uinfo)
    np.testing.assert_array_equal(rows["rbg_to_user"], m)
    assert (rows["rbg_to_user"][:, R - 1] >= 0).all()   # (every TTI uses the last RBG: bit R - 1 of a mask is exercised, bit 63 at 64 RBGs)
    again = logfmt.grant_records_from_rows(rows["tbs_bits"], rows["uinfo"], rows["rbg_to_user"], first_tti=300)
    assert again.tobytes() == recs.tobytes()
    assert "rbg_to_user" not in logfmt.rows_from_grant_records(recs, N_TTIS, U, R, 300, with_map=False)
    with pytest.raises(ValueError):
        logfmt.rows_from_grant_records(recs, N_TTIS, U, R, 301)


def test_a_hand_made_list():
    from radiosaber_amd.api import BATCH_GRANT_RECORD
    recs = np.array([(0, 1, 808, 101, 0b0110, 8, 9, 14, 0), (0, 3, 16, 2, 1 << 63, 4, 1, 0, 0), (2, 1, 8 * 100000001, 100000000, 1, 4, 15, 28, 0)],
                    BATCH_GRANT_RECORD)
    assert logfmt.grant_record_lines(recs, [0, 0, 1, 1], first_ts=100, cum_bytes0=[0, 2**33, 0, 5], cum_rbs0=[0, 1, 0, 0]) == [
        f"100 app: 1 cumu_bytes: {2**33 + 101} cumu_rbs: 9 hol_delay: 0 user: 1 slice: 0",
        "100 app: 3 cumu_bytes: 7 cumu_rbs: 4 hol_delay: 0 user: 3 slice: 1",
        f"102 app: 1 cumu_bytes: {2**33 + 101 + 100000000} cumu_rbs: 13 hol_delay: 0 user: 1 slice: 0"]
    rows = logfmt.rows_from_grant_records(recs, 3, 4, 64)
    assert rows["rbg_to_user"][0].tolist() == [-1, 1, 1] + [-1] * 60 + [3] and rows["rbg_to_user"][1].max() == -1
    assert rows["uinfo"][2, 1] == 4 | (15 << 16) | (28 << 24) and rows["tbs_bits"][0, 3] == 16
