"""Bearer records (not gpu): rs_bearer_record, rs_batch_record_bound and rs_batch_run_records are declared, exported and listed; they
are additions to ABI 11 -- the record is 32 bytes in the header and on the device, RsLaunch did not grow and its pinned gaps hold --, and
logfmt.BearerLogWriter.record_lines writes from records what lines() writes from the dense rows of a logged launch."""
import subprocess

import numpy as np

from radiosaber_amd import logfmt
from test_group_run_counted_abi import ROOT, _probe

NEW = ("rs_batch_record_bound", "rs_batch_run_records")
FIELDS = ("tti", "user", "bearer", "bytes", "nprb", "reserved", "hol_delay")


def test_the_symbols_are_exported_and_listed(rs):
    for name in NEW:
        assert hasattr(rs.lib(), name), f"{name}: declared but not exported"
        assert name in rs.api.ABI_SYMBOLS
    assert callable(rs.BatchScheduler.record_bound) and callable(rs.BatchScheduler.run_records)
    assert callable(logfmt.BearerLogWriter.record_lines)
    assert rs.lib().rs_abi_version() == 11


def test_a_null_handle_is_invalid(rs):
    L = rs.lib()
    n = np.zeros(1, np.int64)
    recs = np.zeros(4, rs.api.BEARER_RECORD)
    for rc in (L.rs_batch_record_bound(None), L.rs_batch_run_records(None, 1, 4, recs.ctypes.data, n.ctypes.data_as(L.rs_batch_run_records.argtypes[4]))):
        assert rc == -1
        assert "null" in L.rs_last_error().decode()


def test_the_record_is_32_bytes(rs, tmp_path):
    """A C probe against the public header: the prototypes (an incompatible pointer type stops the build under -Werror), the record's
    size and field offsets, the version; the numpy dtype of the Python surface and the device's twin are the same record."""
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "radiosaber_hip.h"\n'
                   'typedef int (*bound_fn)(rs_batch*);\n'
                   'typedef int (*run_fn)(rs_batch*, int32_t, int64_t, rs_bearer_record*, int64_t*);\n'
                   'bound_fn f0 = rs_batch_record_bound;\nrun_fn f1 = rs_batch_run_records;\n'
                   'int main(void) { printf("%d %zu", RS_ABI_VERSION, sizeof(rs_bearer_record));\n'
                   + "".join(f'  printf(" %zu", offsetof(rs_bearer_record, {f}));\n' for f in FIELDS) +
                   '  return !f0 || !f1; }\n')
    exe = tmp_path / "probe"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), str(rs.build.LIB), f"-Wl,-rpath,{rs.build.LIB.parent}",
                    "-o", str(exe)], check=True)
    abi, size, *offs = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert abi == 11
    assert size == 32 and offs == [0, 4, 8, 12, 16, 20, 24]
    dt = rs.api.BEARER_RECORD
    assert dt.itemsize == 32 and [dt.fields[n][1] for n in FIELDS] == offs
    dev = _probe(tmp_path, "dev", '  printf("%zu", sizeof(RsBearerRecord));\n'
                 + "".join(f'  printf(" %zu", offsetof(RsBearerRecord, {f}));\n' for f in FIELDS))
    assert [int(x) for x in dev] == [32] + offs


def test_the_launch_block_did_not_move(tmp_path):
    """The pinned gaps of RsLaunch (tests/test_group_*_abi.py) as they were: the record block rides in a pointer pair no batch launch used."""
    out = _probe(tmp_path, "gaps",
                 '  printf("%zu %zu %zu %zu %zu %zu\\n", offsetof(RsLaunch, grp_cbytes) - offsetof(RsLaunch, prio_sum),\n'
                 '    offsetof(RsLaunch, grp_qavg) - offsetof(RsLaunch, grp_cbytes), offsetof(RsLaunch, grp_in) - offsetof(RsLaunch, grp_qavg),\n'
                 '    offsetof(RsLaunch, grp_image) - offsetof(RsLaunch, grp_count), offsetof(RsLaunch, grp_avg) - offsetof(RsLaunch, grp_prb_stride),\n'
                 '    sizeof(RsLaunch) - offsetof(RsLaunch, grp_avg));')
    assert [int(x) for x in out] == [8, 32, 48, 8, 8, 40]


def _hand_made(rs, pf_flows):
    """Six TTIs of 4 users (slices 0, 0, 1, 1), bearers (app ids) 0/1 of user 0, 2/3 of user 1, 4 of user 2, 5/6 of user 3.  TTI 0: user
    0 alone, a split grant; TTI 1: users 1 and 3, user 3 split; TTI 2: nothing; TTI 3: user 0's bearer 0 alone and user 2; TTI 4: nothing;
    TTI 5: user 1 split.  InternetFlow flows on (0, 0), (0, 1) and (1, 1): starts in TTIs 0, 0, 1, 2 (a TTI without a record) and 4, ends
    in TTIs 0, 3 and 5.  -> the credits as tuples (tti, user, bearer, bytes, nprb, hol), flows, done."""
    ticks = [0.1]
    for _ in range(5):
        ticks.append(ticks[-1] + 0.001)
    credits = [(0, 0, 1, 700, 8, 0.0), (0, 0, 0, 45, 8, 0.00001),
               (1, 1, 1, 1200, 16, 0.0040000000000000036), (1, 3, 1, 90, 4, 0.001), (1, 3, 0, 10, 4, 0.0),
               (3, 0, 0, 2**31 - 1 - 45, 24, 0.0030000000000000027), (3, 2, 0, 333, 12, 0.0),
               (5, 1, 1, 80, 8, 0.002), (5, 1, 0, 100000000, 8, 0.0)]
    if pf_flows:  # (scheduler 1: each flow its own PRBs)
        credits = [(t, u, k, by, nprb + 4 * k, hol) for t, u, k, by, nprb, hol in credits]
    flows = {(0, 0): (np.array([ticks[0], ticks[2]]), np.array([0, 1]), np.array([45, 300])),
             (0, 1): (np.array([ticks[0]]), np.array([0]), np.array([692])),
             (1, 1): (np.array([ticks[1], ticks[4] - 0.0004]), np.array([0, 0]), np.array([1192, 72]))}
    done = {(0, 0): (np.array([0, 3], np.int32), np.array([ticks[0], ticks[3]])),
            (0, 1): (np.array([0], np.int32), np.array([ticks[0]])),
            (1, 1): (np.array([-1, 5], np.int32), np.array([-1.0, ticks[5]]))}
    return ticks, credits, flows, done


def _both_forms(rs, credits, n_ttis, U):
    by, hol, rbs = np.zeros((n_ttis, U, 2), np.int64), np.zeros((n_ttis, U, 2)), np.zeros((n_ttis, U, 2), np.int64)
    for t, u, k, b, nprb, h in credits:
        by[t, u, k], hol[t, u, k], rbs[t, u, k] = b, h, nprb
    records = np.array([(t, u, k, b, nprb, 0, h) for t, u, k, b, nprb, h in credits], rs.api.BEARER_RECORD)
    return by, hol, rbs, records


def test_record_lines_are_the_log_lines(rs):
    """lines() and record_lines() are two front ends of one line writer (_launch_lines): what differs, and what this compares, is how
    the launch's credits are gathered -- from dense rows, or from records with batch-wide TTI numbers.  The writer itself (counters,
    ipflow interleaving, formats) is pinned through lines() by tests/test_flow_logfmt.py and, on the GPU, by tests/test_gpu_flow_log.py's run_experiment case;
    the assertions on single lines below pin it here once more."""
    app_of = np.array([[0, 1], [2, 3], [4, -1], [5, 6]])
    u2s = [0, 0, 1, 1]
    for pf_flows in (False, True):
        for flow_format in (False, True):
            ticks, credits, flows, done = _hand_made(rs, pf_flows)
            by, hol, rbs, records = _both_forms(rs, credits, 6, 4)
            # the device may hand the places of one TTI out in any order; the host sorts -- the writer must not depend on it either way
            records = records[np.lexsort((records["bearer"] if pf_flows else -records["bearer"], records["user"], records["tti"]))]
            kw = dict(pf_flows=pf_flows, flows=flows, first_ts=100, cum_bytes0=np.full((4, 2), 2**33), cum_rbs0=np.full((4, 2), 7),
                      flow_format=flow_format)
            for launches in ([6], [1, 2, 3], [3, 3]):   # (a launch boundary in front of, behind and between the TTIs without a record)
                a, b = logfmt.BearerLogWriter(app_of, u2s, **kw), logfmt.BearerLogWriter(app_of, u2s, **kw)
                want, got, t0 = [], [], 0
                for n in launches:
                    want += a.lines(by[t0:t0 + n], hol[t0:t0 + n], rbs[t0:t0 + n], ticks[t0], done)
                    mine = records[(records["tti"] >= t0) & (records["tti"] < t0 + n)]
                    got += b.record_lines(mine, ticks[t0], n, done)
                    t0 += n
                assert got == want, (pf_flows, flow_format, launches)
                assert len(want) == 9 + 5 + 4 and a.tti == b.tti == 6
            order = (0, 1) if pf_flows else (1, 0)
            first = [ln for ln in want if ln.startswith("100 ")]
            assert [int(ln.split()[2]) for ln in first] == [app_of[0, k] for k in order]      # the split grant in the reference's loop order
            assert want[0].startswith("ipflow start") and want[1].startswith("ipflow start")  # ... behind the TTI's ipflow start lines
            assert any(ln.startswith("ipflow end app: 1 ") for ln in want[:6])
            assert first[0].startswith("100 flow: " if flow_format else "100 app: ") and (len(first[0].split()) == 13) == (not flow_format)
            assert sum(ln.startswith("102 ") or ln.startswith("104 ") for ln in want) == 0    # the TTIs without a record
            assert f"cumu_bytes: {2**33 + 45 + 2**31 - 1 - 45} " in " ".join(ln for ln in want if ln.startswith("103 "))


def test_record_lines_refuse_a_record_of_another_launch(rs):
    w = logfmt.BearerLogWriter(np.array([[0, 1]]), [0])
    rec = np.array([(3, 0, 1, 10, 2, 0, 0.0)], rs.api.BEARER_RECORD)
    try:
        w.record_lines(rec, 0.1, 3)
    except ValueError as e:
        assert "TTI 3" in str(e)
    else:
        raise AssertionError("a record outside the launch's TTIs was accepted")
    assert w.record_lines(rec, 0.1, 4) == ["103 app: 1 cumu_bytes: 10 cumu_rbs: 2 hol_delay: 0 user: 0 slice: 0"]
