"""Grant records (not gpu): rs_grant_record, rs_group_grant_bound and rs_group_run_records_at are declared, exported and listed; they are
additions to ABI 11 -- the record is 32 bytes, the slot header took the records' word out of its padding at 104, RsLaunch did not grow,
the seventh form is what it was --, and logfmt.run_record_lines writes from records what logfmt.stderr_lines writes from outputs."""
import subprocess

import numpy as np

from radiosaber_amd import logfmt
from test_group_run_counted_abi import ROOT, _probe

NEW = ("rs_group_grant_bound", "rs_group_run_records_at")


def test_the_symbols_are_exported_and_listed(rs):
    for name in NEW + ("rs_group_run_counted_at",):
        assert hasattr(rs.lib(), name), f"{name}: declared but not exported"
        assert name in rs.api.ABI_SYMBOLS
    assert isinstance(rs.GroupScheduler.grant_bound, property)
    assert callable(logfmt.run_record_lines)
    L = rs.lib()
    assert L.rs_group_grant_bound(None) == -1 and "null" in L.rs_last_error().decode()
    assert L.rs_group_run_records_at(None, 1, None, None, 1, None, None, None, 8, None, None) == -1 and "null" in L.rs_last_error().decode()


def test_the_record_is_32_bytes(rs, tmp_path):
    """A C probe against the public header: the prototypes (an incompatible pointer type stops the build under -Werror), the record's
    size and field offsets, the version; and the numpy dtype of the Python surface is the same record."""
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "radiosaber_hip.h"\n'
                   'typedef int (*bound_fn)(const rs_group*);\n'
                   'typedef int (*run_fn)(rs_group*, int32_t, const int32_t*, const rs_tti_in*, int32_t, const double*, const int32_t*, rs_tti_out*,\n'
                   '                      int32_t, rs_grant_record*, int32_t*);\n'
                   'bound_fn f0 = rs_group_grant_bound;\nrun_fn f1 = rs_group_run_records_at;\n'
                   'int main(void) { printf("%d %zu %zu %zu %zu %zu %zu %zu\\n", RS_ABI_VERSION, sizeof(rs_grant_record), offsetof(rs_grant_record, pos),\n'
                   '    offsetof(rs_grant_record, user_id), offsetof(rs_grant_record, bytes), offsetof(rs_grant_record, nprb),\n'
                   '    offsetof(rs_grant_record, cum_bytes), offsetof(rs_grant_record, cum_rbs));\n'
                   '  return !f0 || !f1; }\n')
    exe = tmp_path / "probe"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), str(rs.build.LIB), f"-Wl,-rpath,{rs.build.LIB.parent}",
                    "-o", str(exe)], check=True)
    abi, size, *offs = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert abi == 11 and rs.lib().rs_abi_version() == 11
    assert size == 32 and offs == [0, 4, 8, 12, 16, 24]
    dt = rs.api.GRANT_RECORD
    assert dt.itemsize == 32 and [dt.fields[n][1] for n in ("pos", "user_id", "bytes", "nprb", "cum_bytes", "cum_rbs")] == offs


def test_the_slot_header_kept_its_size_and_its_words(tmp_path):
    """RsGroupCell took one more word out of its padding, at 104 behind run_no_out; every pinned word is where it was; RsLaunch is what it
    was: five pointers behind grp_avg, the record block travels in grp_sent / grp_sent_stride; the device's record is the ABI's."""
    out = _probe(tmp_path, "hdr",
                 '  printf("%zu %d %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(RsGroupCell), RS_GROUP_HDR_BYTES, offsetof(RsGroupCell, image_mode),\n'
                 '    offsetof(RsGroupCell, in_uid), offsetof(RsGroupCell, now), offsetof(RsGroupCell, run_ttis), offsetof(RsGroupCell, run_table),\n'
                 '    offsetof(RsGroupCell, run_out_step), offsetof(RsGroupCell, run_no_out), offsetof(RsGroupCell, run_rec_cap),\n'
                 '    sizeof(RsLaunch) - offsetof(RsLaunch, grp_avg), offsetof(RsLaunch, grp_crbs) - offsetof(RsLaunch, grp_cbytes),\n'
                 '    sizeof(RsGrantRecord), offsetof(RsGrantRecord, cum_bytes));')
    size, hdr, off_mode, off_uid, off_now, off_ttis, off_table, off_step, off_no_out, off_rec, tail, pair, rec, rec_cum = (int(x) for x in out)
    assert size == hdr == 128
    assert (off_mode, off_uid, off_now) == (72, 76, 80)
    assert (off_ttis, off_table, off_step, off_no_out) == (88, 92, 96, 100)
    assert off_rec == 104                                     # the next word of what was padding
    assert tail == 5 * 8                                      # no RsLaunch field was added
    assert pair == 8
    assert (rec, rec_cum) == (32, 16)


def test_the_seventh_form_is_what_it_was(tmp_path):
    """rs_group_form(6), field for field what tests/test_group_run_counted_abi.py::test_the_seventh_form says: no new form row, no
    RS_GROUP_SET_SENT in the row's sets, no run-time builds."""
    out = _probe(tmp_path, "form",
                 '  constexpr RsGroupForm f = rs_group_form(6), run = rs_group_form(RS_GROUP_RUN);\n'
                 '  static_assert(RS_GROUP_FORMS == 7 && RS_GROUP_RUN_COUNTED == 6, "");\n'
                 '  printf("%s %d%d%d%d%d %u %u %d %d %u", f.stem, f.res, f.que, f.cnt, f.flow, f.run, f.sets, run.sets | RS_GROUP_SET_COUNTERS, f.jit_flags,\n'
                 '         f.scheds == run.scheds, f.sets & RS_GROUP_SET_SENT);\n'
                 '  for (int s : {1, 7, 8, 9, 10, 11, 101, 103}) printf(" %d", (int)rs_group_form_serves(6, s));\n'
                 '  for (int s : {1, 7, 8, 9, 10, 11, 101, 103}) printf(" %d", (int)rs_group_form_builds(6, s));\n'
                 '  printf(" %d%d", (int)rs_group_kernel_exists(6, 9, 0), (int)rs_group_kernel_exists(6, 10, 0));')
    assert out[0] == "rs_group_run_counted_kernel"
    assert out[1] == "10101"
    assert out[2] == out[3]
    assert int(out[4]) == 8 | 16 | 64 | 256 and out[5] == "1" and out[6] == "0"
    assert [int(x) for x in out[7:15]] == [1, 0, 1, 1, 1, 0, 1, 1]
    assert [int(x) for x in out[15:23]] == [0] * 8
    assert out[23] == "10"


def _hand_made(rs):
    """Three TTIs of 5 users in slices 0, 0, 1, 1, 2 with 4 RBGs of 2 PRBs: user 3 is served in TTIs 0 and 2, TTI 1 has no grant at all,
    user 0's block of TTI 2 is 7 bits -- no byte, no line --, and user 4's is above the cap of 1e8 bytes."""
    tbs = np.array([[0, 800, 0, 1608, 0], [0, 0, 0, 0, 0], [7, 0, 0, 4000, 900000000]], np.int64)
    rbg = np.array([[1, 3, 3, -1], [-1, -1, -1, -1], [0, 3, 4, 4]], np.int32)
    nprb = np.array([[0, 2, 0, 4, 0], [0, 0, 0, 0, 0], [2, 0, 0, 2, 4]], np.int32)
    cb0 = np.array([5, 2**33 + 1, 7, 2**40, 11], np.int64)
    cr0 = np.array([1, 2**32 + 5, 3, 9, 2**35], np.int64)
    cb, cr = cb0.copy(), cr0.copy()
    records = []
    for t in range(3):
        rows = []
        for u in range(5):
            b = min(int(tbs[t, u]) // 8, 100000000)
            if b:
                cb[u] += b
                cr[u] += int(nprb[t, u])
                rows.append((u, u, b, int(nprb[t, u]), int(cb[u]), int(cr[u])))
        records.append(np.array(rows, rs.api.GRANT_RECORD))
    return tbs, rbg, nprb, cb0, cr0, records


def test_record_lines_are_the_log_lines(rs):
    tbs, rbg, nprb, cb0, cr0, records = _hand_made(rs)
    slices = [0, 0, 1, 1, 2]
    assert [len(r) for r in records] == [2, 0, 2]
    for pf_format in (False, True):
        for use_nprb in (nprb, None):   # (stderr_lines counts the PRBs from the owner map when it is given none: the same here)
            want = logfmt.stderr_lines(tbs, rbg, slices, 2, first_ts=100, cum_bytes0=cb0, cum_rbs0=cr0, nprb=use_nprb, pf_format=pf_format)
            got = logfmt.run_record_lines(records, slices, first_ts=100, pf_format=pf_format)
            assert got == want and len(got) == 4
    assert logfmt.run_record_lines(records, slices)[0] == f"100 app: 1 cumu_bytes: {2**33 + 101} cumu_rbs: {2**32 + 7} hol_delay: 0 user: 1 slice: 0"
    assert logfmt.run_record_lines(records, slices, first_ts=7, pf_format=True)[-1] == f"9 flow: 4 cumu_bytes: {100000011} cumu_rbs: {2**35 + 4} hol_delay: 0"
    # user 3, served twice: its second line carries both credits
    assert f"102 app: 3 cumu_bytes: {2**40 + 201 + 500} cumu_rbs: {9 + 4 + 2} hol_delay: 0 user: 3 slice: 1" in logfmt.run_record_lines(records, slices)


def test_record_lines_name_the_user_id(rs):
    """A call that names its users: the line's app and user are the record's user_id, the slice is that user's."""
    rec = np.array([(0, 4, 10, 2, 110, 12), (1, 9, 20, 4, 220, 14)], rs.api.GRANT_RECORD)
    slices = [0] * 5 + [1] * 4 + [2] * 3
    assert logfmt.run_record_lines([rec], slices, first_ts=5) == [
        "5 app: 4 cumu_bytes: 110 cumu_rbs: 12 hol_delay: 0 user: 4 slice: 0", "5 app: 9 cumu_bytes: 220 cumu_rbs: 14 hol_delay: 0 user: 9 slice: 2"]
