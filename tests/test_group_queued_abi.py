"""Resident bearers of a group's cells (not gpu): rs_group_set_bearers / rs_group_get_bearers / rs_group_schedule_tti_queued are
declared, exported and listed, additions to ABI 11 with no struct moved; and the inputs of the oracle comparison
(tests/test_gpu_group_queued.py) bind: run through the oracle alone, they credit bearers less than the grant, split grants over a
user's two bearers, meet users with data in both bearers and in one of two, and leave cells without an active user.

The scenario lives here because both files need it: `oracle_run` steps one oracle cell per group cell through DoSchedule() with
queues (rso_cell_step_queues) and records, per TTI and cell, what a binding would pass to rs_group_schedule_tti_queued -- the active
users, their m_dataToTransmit words, the rand() pair when the oracle drew one -- and what the oracle answered."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from conftest import synth_cqi

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "radiosaber_amd" / "csrc"
NEW = ("rs_group_set_bearers", "rs_group_get_bearers", "rs_group_schedule_tti_queued")
HIST = (152600, 56656, 270880, 2088792, 3509504, 1595568, 4145392, 5295816, 1903424,
        6890232, 4770864, 2842552, 3579624, 96000, 1227696)
INFINITE = 100000000
FIELDS = ("target_rbs", "quota_rbgs", "rbg_to_user", "user_nprb", "user_final_cqi", "user_mcs", "user_tbs_bits")
PER_USER = ("user_nprb", "user_final_cqi", "user_mcs", "user_tbs_bits")


# ---------------------------------------------------------------------------------------------------------------------------
# the scenario of the oracle comparison
# ---------------------------------------------------------------------------------------------------------------------------

UES, R_SMALL, G_SMALL, CELLS, TTIS, GRID_EVERY = [5, 4, 3], 8, 2, 3, 80, 10
STATE_AT = (1, 2, 40, 80)  # averages are compared after these TTIs (counted from 1)
ROWS = {"Q-": (2, 0), "-Q": (0, 2), "QQ": (2, 2), "IQ": (1, 2), "I-": (1, 0)}


def bearer_kinds(sched, cell, ues=UES):
    """[U][2] bearer kinds (0 none, 1 InfiniteBuffer, 2 finite queue; index = priority) of one cell: "Q-", "QQ" and "IQ" rows mixed.
    Scheduler 7: every slice's first user is an "IQ" row, so that the served slice is never empty.  Otherwise cell 1 holds finite
    bearers only -- it is the cell that falls idle."""
    U = sum(ues)
    first = np.concatenate([[0], np.cumsum(ues)])[:-1]
    cycle = ["Q-", "QQ", "IQ", "QQ", "-Q"] if (sched == 7 or cell != 1) else ["Q-", "QQ", "QQ", "-Q"]
    kinds = np.array([ROWS[cycle[(u + cell) % len(cycle)]] for u in range(U)], np.uint8)
    if sched == 7:
        kinds[first] = ROWS["IQ"]
    return kinds


def arrivals(rng, kinds, ticks, busy):
    """Per finite bearer, bursts at TTI starts: mostly a short last packet (a queue below one grant), now and then full packets (a
    queue of several grants).  busy: the chance of a burst per TTI."""
    out = {}
    for u, b in zip(*np.nonzero(kinds == 2)):
        when = np.nonzero(rng.random(len(ticks)) < busy)[0]
        if len(when) == 0:
            continue
        n_full = (rng.random(len(when)) < 0.15).astype(np.int32) * rng.integers(1, 3, len(when)).astype(np.int32)
        last = rng.integers(20, 400, len(when)).astype(np.int32)
        out[(int(u), int(b))] = (ticks[when], n_full, last)
    return out


def oracle_run(oracle, sched, ues=UES, R=R_SMALL, G=G_SMALL, K=CELLS, n_tti=TTIS, grid_every=GRID_EVERY, seed=0, busy=None, state_at=STATE_AT):
    """-> dict(ticks, kinds [K], steps [n_tti][K], state {tti: [K] avg [U][2]}); a step is a dict: ids (the active users, ascending),
    data [n][2], required_rbs [n] (sched 7), rand (the pair or None), cqi [n][R], epoch, out (the oracle's rso_tti_out)."""
    U = sum(ues)
    ticks = oracle.clock_ticks(100, n_tti)
    rng = np.random.default_rng(4200 + 10 * sched + seed)
    cells, kinds, rngs, twins = [], [], [], []
    for k in range(K):
        cell = oracle.Cell(ues, R, G, sched)
        kd = bearer_kinds(sched, k, ues)
        cell.enable_queues(kd)
        p = busy if busy is not None else (0.04 if (k == 1 and sched != 7) else 0.3)
        for (u, b), (t, nf, la) in arrivals(rng, kd, ticks, p).items():
            cell.set_arrivals(u, b, t, nf, la)
        cells.append(cell)
        kinds.append(kd)
        rngs.append(oracle.Rng(77 + k))
        twins.append(oracle.Rng(77 + k))
    steps, state = [], {}
    grids = [None] * K
    for t in range(n_tti):
        row = []
        for k in range(K):
            if t % grid_every == 0:
                grids[k] = synth_cqi(9000 + 131 * sched + 17 * t + k + seed, (U, R), HIST)
                cells[k].set_cqi(grids[k])
            out = cells[k].new_out()
            rc = cells[k].step_queues(float(ticks[t]), rngs[k], out)
            assert rc == 0, f"rso_cell_step_queues rc = {rc}"
            act, data, req = cells[k].gates()
            ids = np.nonzero(act)[0].astype(np.int32)
            pair = None
            if sched != 7 and len(ids):  # RBsAllocation ran and drew its two values (:160-165)
                pair = (twins[k].rand(), twins[k].rand())
            row.append(dict(ids=ids, data=data[ids].copy(), required_rbs=np.minimum(req[ids], 2**31 - 1).astype(np.int32), rand=pair,
                            cqi=grids[k][ids].copy(), epoch=1 + t // grid_every, out=out))
        steps.append(row)
        if t + 1 in state_at:
            state[t + 1] = [c.bearer_state()["avg_rate"].copy() for c in cells]
    for k in range(K):  # the twin generators followed the oracle's: the same number of values was drawn
        assert rngs[k].rand() == twins[k].rand()
    return dict(ticks=ticks, kinds=kinds, steps=steps, state=state)


def credit(tbs_bits, data):
    """DoStopSchedule's loop for one user: bytes per bearer."""
    available, sent = int(tbs_bits) // 8, [0, 0]
    for b in (1, 0):
        if available <= 0:
            break
        if data[b] > 0:
            sent[b] = min(available, int(data[b]))
            available -= sent[b]
    return sent


def binding_counts(run):
    """What the inputs exercised, from the oracle's records alone."""
    n = dict(less=0, split=0, both=0, one_of_two=0, idle=0, infinite=0)
    for row in run["steps"]:
        for k, st in enumerate(row):
            kd = run["kinds"][k]
            n["idle"] += len(st["ids"]) == 0
            for i, u in enumerate(st["ids"]):
                d, tbs = st["data"][i], st["out"].user_tbs_bits[u]
                sent = credit(tbs, d)
                n["less"] += any(0 < s < tbs // 8 for s in sent)
                n["split"] += sent[0] > 0 and sent[1] > 0
                n["both"] += d[0] > 0 and d[1] > 0
                n["one_of_two"] += bool(kd[u, 0] and kd[u, 1] and (d[0] > 0) != (d[1] > 0))
                n["infinite"] += INFINITE in d
    return n


@pytest.mark.parametrize("sched", [8, 9, 7, 103])
def test_the_inputs_bind(oracle, sched):
    n = binding_counts(oracle_run(oracle, sched))
    assert n["less"] > 0, "no bearer was credited less than tbs_bits / 8"
    assert n["split"] > 0, "no grant was split over both bearers of a user"
    assert n["both"] > 0, "no user had data in both bearers at scan time"
    assert n["one_of_two"] > 0, "no user with two bearers had data in only one"
    assert n["infinite"] > 0, "no InfiniteBuffer bearer was scheduled"
    if sched != 7:
        assert n["idle"] > 0, "no TTI in which a cell had no active user"


def test_the_many_bearers_inputs_bind(oracle):
    """The 2 x 350-user case of the gpu file (four one-RBG grants per cell and TTI: too few for a split to be sure of): its inputs
    credit less than the grant and meet users with data in both bearers and in one of two as well."""
    n = binding_counts(oracle_run(oracle, 9, ues=[350, 350], R=4, G=2, K=2, n_tti=12, grid_every=5, seed=3, busy=0.5, state_at=(12,)))
    assert n["less"] > 0 and n["both"] > 0 and n["one_of_two"] > 0, n


# ---------------------------------------------------------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------------------------------------------------------

def test_the_three_prototypes_compile_and_nothing_moved(rs, tmp_path):
    """A C probe against the public header: assigning each entry point to a pointer of the documented type checks the prototype
    (-Werror: an incompatible pointer type stops the build); then the version and the three struct sizes."""
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "radiosaber_hip.h"\n'
                   'typedef int (*set_fn)(rs_group*, int32_t, const uint8_t*, const double*, double);\n'
                   'typedef int (*get_fn)(rs_group*, int32_t, double*, int32_t*, double*);\n'
                   'typedef int (*queued_fn)(rs_group*, int32_t, const int32_t*, const rs_tti_in*, rs_tti_out*, const double*,\n'
                   '                         const int32_t* const*);\n'
                   'set_fn f0 = rs_group_set_bearers;\nget_fn f1 = rs_group_get_bearers;\nqueued_fn f2 = rs_group_schedule_tti_queued;\n'
                   'int main(void) { printf("%d %zu %zu %zu\\n", RS_ABI_VERSION, sizeof(rs_config), sizeof(rs_tti_in), sizeof(rs_tti_out));\n'
                   '  return !(f0 && f1 && f2); }\n')
    exe = tmp_path / "probe"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), str(rs.build.LIB), f"-Wl,-rpath,{rs.build.LIB.parent}",
                    "-o", str(exe)], check=True)  # (linked against the built library: the symbols resolve)
    abi, cfg, tin, tout = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert abi == 11 and rs.lib().rs_abi_version() == 11 and rs.api.RS_ABI_VERSION == 11
    assert (cfg, tin, tout) == (88, 96, 72)
    assert (cfg, tin, tout) == (C.sizeof(rs.api._Config), C.sizeof(rs.api._TtiIn), C.sizeof(rs.api._TtiOut))


def test_the_symbols_are_exported_and_listed(rs):
    for name in NEW:
        assert hasattr(rs.lib(), name), f"{name}: declared but not exported"
        assert name in rs.api.ABI_SYMBOLS
    for method in ("set_bearers", "get_bearers", "schedule_tti_queued"):
        assert callable(getattr(rs.GroupScheduler, method))


def test_null_arguments_are_invalid(rs):
    L = rs.lib()
    assert L.rs_group_set_bearers(None, 0, None, None, 0.0) == -1
    assert L.rs_group_get_bearers(None, 0, None, None, None) == -1
    assert L.rs_group_schedule_tti_queued(None, 1, None, None, None, None, None) == -1
    assert "null" in L.rs_last_error().decode()


def test_the_slot_header_and_the_group_fields_kept_their_places(tmp_path):
    """RsGroupCell is untouched (the queued form needs no new header word); RsLaunch took the queued form's six words in front of its
    group fields, whose places relative to one another and to the end of the block are what the earlier forms' tests pin."""
    src = tmp_path / "hdr.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "rs_device.h"\n'
                   'int main() { printf("%zu %d %zu %zu %zu %zu\\n", sizeof(RsGroupCell), RS_GROUP_HDR_BYTES, offsetof(RsGroupCell, in_uid),\n'
                   '  offsetof(RsGroupCell, now), offsetof(RsLaunch, grp_in) - offsetof(RsLaunch, grp_qavg),\n'
                   '  sizeof(RsLaunch) - offsetof(RsLaunch, grp_avg)); return 0; }\n')
    exe = tmp_path / "hdr"
    subprocess.run(["c++", "-std=c++17", "-Wall", "-Wno-invalid-offsetof", f"-I{CSRC}", str(src), "-o", str(exe)], check=True)
    size, hdr, off_uid, off_now, block, tail = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert size == hdr == 128 and (off_uid, off_now) == (76, 80)
    assert block == 6 * 8 and tail == 5 * 8
