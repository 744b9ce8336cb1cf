"""Resident flows of a scheduler-1 group's cells (not gpu): rs_group_set_flows / rs_group_get_flows / rs_group_schedule_tti_flows are
declared, exported and listed, additions to ABI 11 with no struct moved; the log lines of a flows call; and the inputs of the oracle
comparison (tests/test_gpu_group_flows.py) bind: run through the oracle alone, they make flows leave the competition through the
data_to_transmit gate, give both flows of one user RBGs in one TTI, credit flows more bytes than they had to transmit, leave cells
without a flow and schedule InfiniteBuffer flows.

The scenario lives here because both files need it: `flows_run` steps one oracle cell per group cell through DoSchedule() with
queues (rso_cell_step_queues, which for scheduler 1 races flows: step_pf_flows) and records, per TTI and cell, what a binding would
pass to rs_group_schedule_tti_flows -- the flows with data in RRC-container order, their bearer words and m_dataToTransmit -- and what
the oracle answered.  A driver of its own: scheduler 1 draws no rand() pair, which test_group_queued_abi.oracle_run assumes of every
scheduler but 7.  Bearer rows, arrival bursts, the CQI histogram and the small shape are that file's."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from conftest import synth_cqi
from test_group_queued_abi import CELLS, G_SMALL, HIST, INFINITE, R_SMALL, UES, arrivals, bearer_kinds

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "radiosaber_amd" / "csrc"
NEW = ("rs_group_set_flows", "rs_group_get_flows", "rs_group_schedule_tti_flows")
SCHED_PF = 1
USERS = sum(UES)  # one slice of users on the oracle side; the group's n_users is the largest flow count, 2 * USERS
TTIS, GRID_EVERY = 80, 10
STATE_AT = (1, 2, 40, 80)  # averages and counters are compared after these TTIs (counted from 1)
AVG0, LAST0 = 100000.0, 0.1  # every bearer's initial average (a user's two flows tie: the first maximum decides) and m_lastUpdate
SEED, BUSY, BUSY_IDLE = 3, 0.3, 0.04  # picked on the CPU so that test_the_inputs_bind holds (cell 1 is the cell that falls idle)


def flows_run(oracle, users=USERS, R=R_SMALL, G=G_SMALL, K=CELLS, n_tti=TTIS, grid_every=GRID_EVERY, seed=SEED, busy=None, state_at=STATE_AT):
    """-> dict(ticks, kinds [K], steps [n_tti][K], state / cum_bytes / cum_rbs {tti: [K] [U][2]}); a step is a dict: uid [F] and fb [F]
    (the flows with data: users ascending, bearer 0 before 1), data [F] (m_dataToTransmit of the flow), cqi [F][R] (the user's row per
    position), epoch, out (the oracle's rso_tti_out: rbg_to_user holds flow ids, the per-user fields are indexed by user id)."""
    ticks = oracle.clock_ticks(100, n_tti)
    rng = np.random.default_rng(5100 + seed)
    cells, kinds, rngs = [], [], []
    for k in range(K):
        cell = oracle.Cell([users], R, G, SCHED_PF)
        kd = bearer_kinds(SCHED_PF, k, [users])
        cell.enable_queues(kd)
        p = busy if busy is not None else (BUSY_IDLE if k == 1 else BUSY)
        for (u, b), (t, nf, la) in arrivals(rng, kd, ticks, p).items():
            cell.set_arrivals(u, b, t, nf, la)
        cells.append(cell)
        kinds.append(kd)
        rngs.append(oracle.Rng(77 + k))
    steps, state, cum_bytes, cum_rbs = [], {}, {}, {}
    grids = [None] * K
    for t in range(n_tti):
        row = []
        for k in range(K):
            if t % grid_every == 0:
                grids[k] = synth_cqi(12000 + 17 * t + k + seed, (users, R), HIST)
                cells[k].set_cqi(grids[k])
            out = cells[k].new_out()
            rc = cells[k].step_queues(float(ticks[t]), rngs[k], out)
            assert rc == 0, f"rso_cell_step_queues rc = {rc}"
            _, data, _ = cells[k].gates()
            uid, fb = (x.astype(np.int32) for x in np.nonzero(data > 0))  # row-major: (user, bearer) ascending
            row.append(dict(uid=uid, fb=fb.astype(np.uint8), data=data[uid, fb].copy(), cqi=grids[k][uid].copy(), epoch=1 + t // grid_every, out=out))
        steps.append(row)
        if t + 1 in state_at:
            bs = [c.bearer_state() for c in cells]
            state[t + 1] = [b["avg_rate"].copy() for b in bs]
            cum_bytes[t + 1] = [b["cum_bytes"].copy() for b in bs]
            cum_rbs[t + 1] = [b["cum_rbs"].copy() for b in bs]
    for k in range(K):  # scheduler 1 draws nothing: the generators are where they started
        assert rngs[k].rand() == oracle.Rng(77 + k).rand()
    return dict(ticks=ticks, kinds=kinds, steps=steps, state=state, cum_bytes=cum_bytes, cum_rbs=cum_rbs)


def flows_binding_counts(run):
    """What the inputs exercised, from the oracle's records alone.  A flow's own transport block is known from the per-user rows
    where it is the only flow of its user that holds RBGs."""
    n = dict(gate=0, both=0, more=0, idle=0, infinite=0)
    for row in run["steps"]:
        for k, st in enumerate(row):
            kd, out = run["kinds"][k], st["out"]
            n["idle"] += len(st["uid"]) == 0
            owners = np.asarray(out.rbg_to_user)
            held = set(int(f) for f in owners if f >= 0)
            n["both"] += sum(1 for f in held if f % 2 == 0 and f + 1 in held)
            n["infinite"] += sum(1 for f in held if kd[f >> 1, f & 1] == 1)
            for u, b, d in zip(st["uid"], st["fb"], st["data"]):
                f = 2 * int(u) + int(b)
                if f not in held or (f ^ 1) in held:
                    continue
                tbs = int(out.user_tbs_bits[u])
                last_rbg = int(np.nonzero(owners == f)[0][-1])
                n["gate"] += tbs >= int(d) * 8 and last_rbg < len(owners) - 1
                n["more"] += tbs // 8 > int(d)
    return n


def test_the_inputs_bind(oracle):
    run = flows_run(oracle)
    n = flows_binding_counts(run)
    assert n["gate"] > 0, "(a) no flow left the competition through the gate with RBGs still to hand out"
    assert n["both"] > 0, "(b) no user whose two flows both received RBGs in one TTI"
    assert n["more"] > 0, "(c) no flow was credited more bytes than its data_to_transmit"
    assert n["idle"] > 0, "(d) no update-only slot: no TTI in which a cell had no flow"
    assert n["infinite"] > 0, "(e) no InfiniteBuffer flow was scheduled"
    assert all(cb.any() for cb in run["cum_bytes"][TTIS]) and sorted(run["cum_bytes"]) == list(STATE_AT)
    assert any(INFINITE in st["data"] for row in run["steps"] for st in row)


def test_the_many_flows_inputs_bind(oracle):
    """The 2 x 350-user case of the gpu file: some call has more than 512 positions, so that the gather strides beyond the
    workgroup's 512 threads, and flows are served in every TTI.  (With equal initial averages and four RBGs per TTI the winners are
    early positions; a position past the 512th that was gathered wrong would win or lose against them and show in the map.)"""
    run = flows_run(oracle, users=350, R=4, G=2, K=2, n_tti=12, grid_every=5, seed=3, busy=0.5, state_at=(12,))
    assert max(len(st["uid"]) for row in run["steps"] for st in row) > 512
    assert all((np.asarray(st["out"].rbg_to_user) >= 0).any() for row in run["steps"] for st in row)


# ---------------------------------------------------------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------------------------------------------------------

def test_the_three_prototypes_compile_and_nothing_moved(rs, tmp_path):
    """A C probe against the public header: assigning each entry point to a pointer of the documented type checks the prototype
    (-Werror: an incompatible pointer type stops the build); then the version and the three struct sizes."""
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "radiosaber_hip.h"\n'
                   'typedef int (*set_fn)(rs_group*, int32_t, const uint8_t*, const double*, double, const int64_t*, const int64_t*);\n'
                   'typedef int (*get_fn)(rs_group*, int32_t, double*, int32_t*, double*, int64_t*, int64_t*);\n'
                   'typedef int (*flows_fn)(rs_group*, int32_t, const int32_t*, const rs_tti_in*, rs_tti_out*, const double*,\n'
                   '                        const uint8_t* const*);\n'
                   'set_fn f0 = rs_group_set_flows;\nget_fn f1 = rs_group_get_flows;\nflows_fn f2 = rs_group_schedule_tti_flows;\n'
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
    for method in ("set_flows", "get_flows", "schedule_tti_flows"):
        assert callable(getattr(rs.GroupScheduler, method))
    from radiosaber_amd import logfmt
    assert callable(logfmt.flows_call_lines)


def test_null_arguments_are_invalid(rs):
    L = rs.lib()
    assert L.rs_group_set_flows(None, 0, None, None, 0.0, None, None) == -1
    assert L.rs_group_get_flows(None, 0, None, None, None, None, None) == -1
    assert L.rs_group_schedule_tti_flows(None, 1, None, None, None, None, None) == -1
    assert "null" in L.rs_last_error().decode()


def test_run_time_builds_do_not_reach_scheduler_1(rs):
    """no queued build for RS_SCHED_PF, as before: the flows form is built in only"""
    buf = C.create_string_buffer(4096)
    assert rs.lib().rs_jit_selfcheck_group_queued(1, 24, R_SMALL, G_SMALL, 512, SCHED_PF, buf, 4096) < 0


def test_the_slot_header_and_the_launch_block_did_not_move(tmp_path):
    """RsGroupCell is untouched, and so is RsLaunch: the flows form reads the bearer stores, the counter stores and the slots' word block
    of the queued and the counted form, whose places the earlier forms' tests pin."""
    src = tmp_path / "hdr.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "rs_device.h"\n'
                   'int main() { printf("%zu %d %zu %zu %zu %zu %zu %zu\\n", sizeof(RsGroupCell), RS_GROUP_HDR_BYTES, offsetof(RsGroupCell, in_uid),\n'
                   '  offsetof(RsGroupCell, now), offsetof(RsLaunch, grp_in) - offsetof(RsLaunch, grp_qavg),\n'
                   '  sizeof(RsLaunch) - offsetof(RsLaunch, grp_avg), offsetof(RsLaunch, grp_qavg) - offsetof(RsLaunch, grp_cbytes),\n'
                   '  offsetof(RsLaunch, grp_cbytes) - offsetof(RsLaunch, prio_sum)); return 0; }\n')
    exe = tmp_path / "hdr"
    subprocess.run(["c++", "-std=c++17", "-Wall", "-Wno-invalid-offsetof", f"-I{CSRC}", str(src), "-o", str(exe)], check=True)
    size, hdr, off_uid, off_now, block, tail, counted, gap = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert size == hdr == 128 and (off_uid, off_now) == (76, 80)
    assert (block, tail, counted, gap) == (6 * 8, 5 * 8, 4 * 8, 8)


def test_the_log_lines_of_a_flows_call(rs):
    """flows_call_lines: one line per credited flow in FlowsToSchedule order -- the call's order: users ascending, bearer 0 before 1 --,
    counters as they are after the credit, against a hand-written expectation (dl-pf-packet-scheduler.cpp:89-96) and against
    BearerLogWriter in its scheduler-1 order."""
    from radiosaber_amd import logfmt as lf
    sc = rs.SliceConfig([2, 2])
    uid = np.array([0, 2, 2, 3], np.int32)
    fb = np.array([1, 0, 1, 0], np.uint8)
    tbs = np.array([0, 328, 12000, 7], np.int32)  # position 0 holds no RBG, position 3 a block below one byte
    hol = np.array([0.25, 0.003, 0.00001, 0.5])
    app = np.array([[0, 4], [1, 5], [2, 6], [3, 7]])
    cb = np.array([[9, 9], [9, 9], [141, 2000], [1040, 17]], np.int64)
    cr = np.array([[1, 1], [1, 1], [4, 12], [8, 6]], np.int64)
    got = lf.flows_call_lines(117, uid, fb, tbs, hol, cb, cr, app, sc.user_to_slice)
    assert got == ["117 app: 2 cumu_bytes: 141 cumu_rbs: 4 hol_delay: 0.003 user: 2 slice: 1",
                   "117 app: 6 cumu_bytes: 2000 cumu_rbs: 12 hol_delay: 1e-05 user: 2 slice: 1"]
    w = lf.BearerLogWriter(app, sc.user_to_slice, pf_flows=True, first_ts=117, cum_bytes0=cb - np.array([[0, 0], [0, 0], [41, 1500], [0, 0]]),
                           cum_rbs0=cr - np.array([[0, 0], [0, 0], [2, 8], [0, 0]]))
    by, hl, rb = np.zeros((1, 4, 2), np.int64), np.zeros((1, 4, 2)), np.zeros((1, 4, 2), np.int64)
    by[0, uid, fb], hl[0, uid, fb] = tbs // 8, hol
    rb[0, 2] = (2, 8)
    assert w.lines(by, hl, rb, 0.117) == got
    assert lf.flows_call_lines(5, None, np.zeros(0, np.uint8), np.zeros(0, np.int32), None, cb, cr, app, sc.user_to_slice) == []
