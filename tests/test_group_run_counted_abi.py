"""Counted runs (not gpu): rs_group_set_avg_counters, rs_group_get_avg_counters and rs_group_run_counted_at are declared, exported and
listed; they are additions to ABI 11 -- no struct moved --, the slot header took its "no outputs" word out of its padding, RsLaunch did
not grow, and the seventh row of rs_group_form is a form without run-time builds whose flag set the builds' front end refuses."""
import ctypes as C
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "radiosaber_amd" / "csrc"
NEW = ("rs_group_set_avg_counters", "rs_group_get_avg_counters", "rs_group_run_counted_at")
SCHEDS = (1, 7, 8, 9, 10, 11, 101, 103)
SHAPE = (4, 40, 13, 4, 512)  # slices, users, RBGs, PRBs per RBG, threads


def test_the_prototypes_compile_and_nothing_moved(rs, tmp_path):
    """A C probe against the public header: assigning each entry point to a pointer of the documented type is what checks the prototype
    (-Werror: an incompatible pointer type stops the build); then the version and the three struct sizes."""
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "radiosaber_hip.h"\n'
                   'typedef int (*set_fn)(rs_group*, int32_t, const int64_t*, const int64_t*);\n'
                   'typedef int (*get_fn)(rs_group*, int32_t, int64_t*, int64_t*);\n'
                   'typedef int (*run_fn)(rs_group*, int32_t, const int32_t*, const rs_tti_in*, int32_t, const double*, const int32_t*, rs_tti_out*);\n'
                   'set_fn f0 = rs_group_set_avg_counters;\nget_fn f1 = rs_group_get_avg_counters;\nrun_fn f2 = rs_group_run_counted_at;\n'
                   'int main(void) { printf("%d %zu %zu %zu\\n", RS_ABI_VERSION, sizeof(rs_config), sizeof(rs_tti_in), sizeof(rs_tti_out));\n'
                   '  return !f0 || !f1 || !f2; }\n')
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
    for method in ("set_avg_counters", "get_avg_counters", "run_counted_at"):
        assert callable(getattr(rs.GroupScheduler, method))


def test_null_arguments_are_invalid(rs):
    L = rs.lib()
    for rc in (L.rs_group_set_avg_counters(None, 0, None, None), L.rs_group_get_avg_counters(None, 0, None, None),
               L.rs_group_run_counted_at(None, 1, None, None, 1, None, None, None)):
        assert rc == -1
        assert "null" in L.rs_last_error().decode()


def _probe(tmp_path, name, body):
    src = tmp_path / f"{name}.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include <cstring>\n#include <initializer_list>\n#include "rs_device.h"\nint main() {\n' + body + '\n  return 0; }\n')
    exe = tmp_path / name
    subprocess.run(["c++", "-std=c++17", "-Wall", "-Wno-invalid-offsetof", f"-I{CSRC}", str(src), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()


def test_the_slot_header_kept_its_size_and_its_words(tmp_path):
    """RsGroupCell took one word -- "this run writes no outputs" -- out of its padding, behind run_out_step; RsLaunch is what it was: five
    pointers behind grp_avg, and the counters travel in the two pointers the counted form already had."""
    out = _probe(tmp_path, "hdr",
                 '  printf("%zu %d %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(RsGroupCell), RS_GROUP_HDR_BYTES, offsetof(RsGroupCell, image_mode),\n'
                 '    offsetof(RsGroupCell, in_uid), offsetof(RsGroupCell, now), offsetof(RsGroupCell, run_ttis), offsetof(RsGroupCell, run_table),\n'
                 '    offsetof(RsGroupCell, run_out_step), offsetof(RsGroupCell, run_no_out), sizeof(RsLaunch) - offsetof(RsLaunch, grp_avg),\n'
                 '    offsetof(RsLaunch, grp_crbs) - offsetof(RsLaunch, grp_cbytes));')
    size, hdr, off_mode, off_uid, off_now, off_ttis, off_table, off_step, off_no_out, tail, pair = (int(x) for x in out)
    assert size == hdr == 128
    assert (off_mode, off_uid, off_now) == (72, 76, 80)       # where the parent commit has them
    assert (off_ttis, off_table, off_step) == (88, 92, 96)    # the run's words
    assert off_no_out == 100                                  # the first word of what was padding
    assert tail == 5 * 8                                      # no RsLaunch field was added
    assert pair == 8


def test_the_seventh_form(tmp_path):
    """rs_group_form(6): the stem, res = cnt = run, the run row's pointers plus the counters, the run row's schedulers; and every flag
    set that named a form still names it."""
    out = _probe(tmp_path, "form",
                 '  constexpr RsGroupForm f = rs_group_form(6), run = rs_group_form(RS_GROUP_RUN);\n'
                 '  static_assert(RS_GROUP_FORMS == 7 && RS_GROUP_RUN_COUNTED == 6, "");\n'
                 '  printf("%s %d%d%d%d%d %u %u %d %d", f.stem, f.res, f.que, f.cnt, f.flow, f.run, f.sets, run.sets | RS_GROUP_SET_COUNTERS, f.jit_flags, f.scheds == run.scheds);\n'
                 '  for (int s : {1, 7, 8, 9, 10, 11, 101, 103}) printf(" %d", (int)rs_group_form_serves(6, s));\n'
                 '  for (int s : {1, 7, 8, 9, 10, 11, 101, 103}) printf(" %d", (int)rs_group_form_builds(6, s));\n'
                 '  for (int fl : {8, 8 | 16, 8 | 32, 8 | 128, 8 | 32 | 64, 8 | 16 | 256, 8 | 16 | 64 | 256, 0, 16, 8 | 16 | 32, 8 | 64, 1 | 4 | 8 | 16 | 256})\n'
                 '    printf(" %d", rs_group_form_of_flags(fl));\n'
                 '  printf(" %d%d", (int)rs_group_kernel_exists(6, 9, 0), (int)rs_group_kernel_exists(6, 10, 0));')
    assert out[0] == "rs_group_run_counted_kernel"
    assert out[1] == "10101"                               # res, cnt and run
    assert out[2] == out[3]                                # the run row's sets plus RS_GROUP_SET_COUNTERS
    assert int(out[4]) == 8 | 16 | 64 | 256 and out[5] == "1"
    assert [int(x) for x in out[6:14]] == [1, 0, 1, 1, 1, 0, 1, 1]   # schedulers 1, 8, 9, 10, 101, 103
    assert [int(x) for x in out[14:22]] == [0] * 8                    # no run-time build of this form, for any scheduler
    #  the six forms' flag sets as before, the new one, and sets that name no form
    assert [int(x) for x in out[22:34]] == [0, 1, 2, 3, 4, 5, 6, -1, -1, -1, -1, 5]
    assert out[34] == "10"                                 # <9, 0> exists, <10, 0> does not: the run row's EPT rule


def test_no_cache_file_for_the_new_flag_set(rs, monkeypatch, tmp_path):
    """rs_jit_cache_file and rs_jit_cache_warm refuse 8 | 16 | 64 | 256 for every scheduler, lean or not; the warm call says why."""
    monkeypatch.setenv("RS_JIT_CACHE_DIR", str(tmp_path))
    L = rs.lib()
    for sched in SCHEDS:
        for lean in (0, 4):
            buf = C.create_string_buffer(512)
            assert L.rs_jit_cache_file(*SHAPE, sched, 8 | 16 | 64 | 256 | lean, buf, 512) == 0 and buf.value == b""
            err = C.create_string_buffer(512)
            assert L.rs_jit_cache_warm(*SHAPE, sched, 8 | 16 | 64 | 256 | lean, err, 512) == -1
            assert "rs_group_run_counted_kernel" in err.value.decode() and "no run-time build" in err.value.decode()
    assert not list(tmp_path.iterdir())
