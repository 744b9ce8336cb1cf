"""Counted bearers of a group's cells (not gpu): rs_group_set_counters / rs_group_get_counters / rs_group_schedule_tti_counted are
declared, exported and listed, additions to ABI 11 with no struct moved; and the inputs of the oracle comparison
(tests/test_gpu_group_counted.py) bind: run through the oracle alone, they split grants over two bearers, credit less than the grant,
serve users one of whose bearers has no data and earns no RBs, leave cells without an active user and make the two bearers' RB
counters differ.

The scenario is tests/test_group_queued_abi.py's (its constants and helpers are imported, not restated); `counted_run` is
`oracle_run` with the oracle's per-bearer counters recorded beside the averages, and with an idle cell under scheduler 7 as well."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from conftest import synth_cqi
from test_group_queued_abi import CELLS, G_SMALL, HIST, R_SMALL, UES, arrivals, bearer_kinds, credit

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "radiosaber_amd" / "csrc"
NEW = ("rs_group_set_counters", "rs_group_get_counters", "rs_group_schedule_tti_counted")
TTIS, GRID_EVERY = 80, 10
STATE_AT = (1, 2, 40, 80)  # averages and counters are compared after these TTIs (counted from 1)
SCHEDS = [8, 9, 7, 103, 101]


def counted_run(oracle, sched, ues=UES, R=R_SMALL, G=G_SMALL, K=CELLS, n_tti=TTIS, grid_every=GRID_EVERY, seed=0, busy=None, state_at=STATE_AT):
    """-> dict(ticks, kinds [K], steps [n_tti][K], state / cum_bytes / cum_rbs {tti: [K] [U][2]}); a step as oracle_run's: ids (the
    active users, ascending), data [n][2], required_rbs [n] (sched 7), rand (the pair or None), cqi [n][R], epoch, out."""
    U = sum(ues)
    ticks = oracle.clock_ticks(100, n_tti)
    rng = np.random.default_rng(4200 + 10 * sched + seed)
    cells, kinds, rngs, twins = [], [], [], []
    for k in range(K):
        cell = oracle.Cell(ues, R, G, sched)
        # cell 1 is the cell that falls idle, under scheduler 7 too: finite bearers only (the rows bearer_kinds gives that cell for
        # the other schedulers; an NVS cell has nobody to schedule only when no slice has a packet) and few arrivals
        kd = bearer_kinds(sched if k != 1 else 8, k, ues)
        cell.enable_queues(kd)
        p = busy if busy is not None else (0.04 if k == 1 else 0.3)
        for (u, b), (t, nf, la) in arrivals(rng, kd, ticks, p).items():
            cell.set_arrivals(u, b, t, nf, la)
        cells.append(cell)
        kinds.append(kd)
        rngs.append(oracle.Rng(77 + k))
        twins.append(oracle.Rng(77 + k))
    steps, state, cum_bytes, cum_rbs = [], {}, {}, {}
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
            bs = [c.bearer_state() for c in cells]
            state[t + 1] = [b["avg_rate"].copy() for b in bs]
            cum_bytes[t + 1] = [b["cum_bytes"].copy() for b in bs]
            cum_rbs[t + 1] = [b["cum_rbs"].copy() for b in bs]
    for k in range(K):  # the twin generators followed the oracle's: the same number of values was drawn
        assert rngs[k].rand() == twins[k].rand()
    return dict(ticks=ticks, kinds=kinds, steps=steps, state=state, cum_bytes=cum_bytes, cum_rbs=cum_rbs)


def counted_binding_counts(run):
    """What the inputs exercised, from the oracle's records alone."""
    n = dict(split=0, finite=0, dataless=0, idle=0, rbs_differ=0)
    for row in run["steps"]:
        for k, st in enumerate(row):
            kd = run["kinds"][k]
            n["idle"] += len(st["ids"]) == 0
            for i, u in enumerate(st["ids"]):
                d, tbs = st["data"][i], int(st["out"].user_tbs_bits[u])
                sent = credit(tbs, d)
                n["split"] += sent[0] > 0 and sent[1] > 0
                n["finite"] += sum(sent) < tbs // 8  # the queues took less than the grant: bytes of it are left over
                # served, both bearers exist, one of them has no data: its counters (RBs included) must not move
                n["dataless"] += bool(tbs // 8 > 0 and kd[u, 0] and kd[u, 1] and (d[0] == 0 or d[1] == 0))
    last = max(run["cum_rbs"])
    for k, cr in enumerate(run["cum_rbs"][last]):
        both = (run["kinds"][k] != 0).all(axis=1)
        n["rbs_differ"] += bool((cr[both, 0] != cr[both, 1]).any())
    return n


@pytest.mark.parametrize("sched", SCHEDS)
def test_the_inputs_bind(oracle, sched):
    run = counted_run(oracle, sched)
    n = counted_binding_counts(run)
    assert n["split"] > 0, "no grant was split over both bearers of a user"
    assert n["finite"] > 0, "no credit left bytes of the grant over"
    assert n["dataless"] > 0, "no served user had a bearer without data"
    assert n["idle"] > 0, "no update-only slot: no TTI in which a cell had no active user"
    assert n["rbs_differ"] > 0, "no cell whose two bearers' cum_rbs differ"
    # ... and the counters the GPU tests compare are not trivially zero
    assert all(cb.any() for cb in run["cum_bytes"][TTIS]) and sorted(run["cum_bytes"]) == list(STATE_AT)


def test_the_many_bearers_inputs_bind(oracle):
    """The 2 x 350-user case of the gpu file: more than 512 positions of one call are credited, so that a position beyond the
    workgroup's 512 threads is reached by the strided loop alone."""
    run = counted_run(oracle, 9, ues=[350, 350], R=4, G=2, K=2, n_tti=12, grid_every=5, seed=3, busy=0.5, state_at=(12,))
    assert max(len(st["ids"]) for row in run["steps"] for st in row) > 512
    beyond = sum(int(st["out"].user_tbs_bits[u]) // 8 > 0 for row in run["steps"] for st in row for i, u in enumerate(st["ids"]) if i >= 512)
    assert beyond > 0, "no position past the 512th was granted anything"


# ---------------------------------------------------------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------------------------------------------------------

def test_the_three_prototypes_compile_and_nothing_moved(rs, tmp_path):
    """A C probe against the public header: assigning each entry point to a pointer of the documented type checks the prototype
    (-Werror: an incompatible pointer type stops the build); then the version and the three struct sizes."""
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "radiosaber_hip.h"\n'
                   'typedef int (*set_fn)(rs_group*, int32_t, const int64_t*, const int64_t*);\n'
                   'typedef int (*get_fn)(rs_group*, int32_t, int64_t*, int64_t*);\n'
                   'typedef int (*counted_fn)(rs_group*, int32_t, const int32_t*, const rs_tti_in*, rs_tti_out*, const double*,\n'
                   '                          const int32_t* const*, int32_t* const*);\n'
                   'set_fn f0 = rs_group_set_counters;\nget_fn f1 = rs_group_get_counters;\ncounted_fn f2 = rs_group_schedule_tti_counted;\n'
                   'int main(void) { printf("%d %zu %zu %zu\\n", RS_ABI_VERSION, sizeof(rs_config), sizeof(rs_tti_in), sizeof(rs_tti_out));\n'
                   '  return !(f0 && f1 && f2); }\n')
    exe = tmp_path / "probe"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), str(rs.build.LIB), f"-Wl,-rpath,{rs.build.LIB.parent}",
                    "-o", str(exe)], check=True)  # (linked against the built library: the symbols resolve)
    abi, cfg, tin, tout = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert abi == 11 and rs.lib().rs_abi_version() == 11 and rs.api.RS_ABI_VERSION == 11
    assert (cfg, tin, tout) == (88, 96, 72)


def test_the_symbols_are_exported_and_listed(rs):
    for name in NEW:
        assert hasattr(rs.lib(), name), f"{name}: declared but not exported"
        assert name in rs.api.ABI_SYMBOLS
    for method in ("set_counters", "get_counters", "schedule_tti_counted"):
        assert callable(getattr(rs.GroupScheduler, method))
    assert "sent" in rs.api.TtiResult.__dataclass_fields__
    from radiosaber_amd import logfmt
    assert callable(logfmt.counted_call_lines)


def test_null_arguments_are_invalid(rs):
    L = rs.lib()
    assert L.rs_group_set_counters(None, 0, None, None) == -1
    assert L.rs_group_get_counters(None, 0, None, None) == -1
    assert L.rs_group_schedule_tti_counted(None, 1, None, None, None, None, None, None) == -1
    assert "null" in L.rs_last_error().decode()


def test_the_slot_header_and_the_group_fields_kept_their_places(tmp_path):
    """RsGroupCell is untouched (the counted form needs no header word); RsLaunch took the counted form's four words in front of the
    queued form's six, whose places relative to the group fields and to the end of the block are what the earlier forms' tests pin."""
    src = tmp_path / "hdr.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "rs_device.h"\n'
                   'int main() { printf("%zu %d %zu %zu %zu %zu %zu %zu\\n", sizeof(RsGroupCell), RS_GROUP_HDR_BYTES, offsetof(RsGroupCell, in_uid),\n'
                   '  offsetof(RsGroupCell, now), offsetof(RsLaunch, grp_in) - offsetof(RsLaunch, grp_qavg),\n'
                   '  sizeof(RsLaunch) - offsetof(RsLaunch, grp_avg), offsetof(RsLaunch, grp_qavg) - offsetof(RsLaunch, grp_cbytes),\n'
                   '  offsetof(RsLaunch, grp_cbytes) - offsetof(RsLaunch, prio_sum)); return 0; }\n')
    exe = tmp_path / "hdr"
    subprocess.run(["c++", "-std=c++17", "-Wall", "-Wno-invalid-offsetof", f"-I{CSRC}", str(src), "-o", str(exe)], check=True)
    size, hdr, off_uid, off_now, block, tail, mine, gap = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert size == hdr == 128 and (off_uid, off_now) == (76, 80)
    assert block == 6 * 8 and tail == 5 * 8
    assert mine == 4 * 8 and gap == 8


def test_the_log_lines_of_a_counted_call(rs):
    """counted_call_lines: one line per credited bearer, users ascending by id whatever the call order, bearer 1 before 0, in
    BearerLogWriter's format (checked against a writer fed the same credit)."""
    from radiosaber_amd import logfmt as lf
    sc = rs.SliceConfig([2, 2])
    ids = np.array([3, 0, 2], np.int32)
    sent = np.array([[40, 7], [0, 0], [0, 1500]], np.int32)
    hol = np.array([[0.003, 0.0], [0, 0], [0.5, 0.00001]])
    app = np.array([[0, 4], [1, 5], [2, 6], [3, 7]])
    cb = np.array([[9, 9], [9, 9], [100, 2000], [1040, 17]], np.int64)
    cr = np.array([[1, 1], [1, 1], [4, 12], [8, 6]], np.int64)
    got = lf.counted_call_lines(117, ids, sent, hol, cb, cr, app, sc.user_to_slice)
    assert got == ["117 app: 6 cumu_bytes: 2000 cumu_rbs: 12 hol_delay: 1e-05 user: 2 slice: 1",
                   "117 app: 7 cumu_bytes: 17 cumu_rbs: 6 hol_delay: 0 user: 3 slice: 1",
                   "117 app: 3 cumu_bytes: 1040 cumu_rbs: 8 hol_delay: 0.003 user: 3 slice: 1"]
    w = lf.BearerLogWriter(app, sc.user_to_slice, first_ts=117, cum_bytes0=cb - np.array([[0, 0], [0, 0], [0, 1500], [40, 7]]),
                           cum_rbs0=cr - np.array([[0, 0], [0, 0], [0, 4], [2, 2]]))
    by, hl, rb = np.zeros((1, 4, 2), np.int64), np.zeros((1, 4, 2)), np.zeros((1, 4, 2), np.int64)
    by[0, ids], hl[0, ids] = sent, hol
    rb[0, 2], rb[0, 3] = 4, 2
    assert w.lines(by, hl, rb, 0.117) == got
    assert lf.counted_call_lines(5, None, np.zeros((0, 2), np.int32), None, cb, cr, app, sc.user_to_slice) == []
