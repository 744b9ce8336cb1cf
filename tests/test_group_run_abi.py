"""A run of resident group calls (not gpu): rs_group_run_at is declared, exported and listed; it is an addition to ABI 11 -- no struct
moved --, the slot header of the group kernels took its three new words out of its padding and RsLaunch did not grow."""
import ctypes as C
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "radiosaber_amd" / "csrc"


def test_the_prototype_compiles_and_nothing_moved(rs, tmp_path):
    """A C probe against the public header: assigning the entry point to a pointer of the documented type is what checks the prototype
    (-Werror: an incompatible pointer type stops the build); then the bound, the version and the three struct sizes."""
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "radiosaber_hip.h"\n'
                   'typedef int (*run_at_fn)(rs_group*, int32_t, const int32_t*, const rs_tti_in*, int32_t, const double*, const int32_t*, rs_tti_out*);\n'
                   'run_at_fn f0 = rs_group_run_at;\n'
                   'int main(void) { printf("%d %d %zu %zu %zu\\n", RS_ABI_VERSION, RS_GROUP_MAX_RUN, sizeof(rs_config), sizeof(rs_tti_in), sizeof(rs_tti_out));\n'
                   '  return !f0; }\n')
    exe = tmp_path / "probe"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), str(rs.build.LIB), f"-Wl,-rpath,{rs.build.LIB.parent}",
                    "-o", str(exe)], check=True)  # (linked against the built library: the symbol resolves)
    abi, max_run, cfg, tin, tout = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert abi == 11 and rs.lib().rs_abi_version() == 11 and rs.api.RS_ABI_VERSION == 11
    assert max_run == 64   # >= CQI_INTERVAL = 40
    assert (cfg, tin, tout) == (88, 96, 72)
    assert (cfg, tin, tout) == (C.sizeof(rs.api._Config), C.sizeof(rs.api._TtiIn), C.sizeof(rs.api._TtiOut))


def test_the_symbol_is_exported_and_listed(rs):
    assert hasattr(rs.lib(), "rs_group_run_at"), "rs_group_run_at: declared but not exported"
    assert "rs_group_run_at" in rs.api.ABI_SYMBOLS
    assert callable(rs.GroupScheduler.run_at)


def test_null_arguments_are_invalid(rs):
    L = rs.lib()
    assert L.rs_group_run_at(None, 1, None, None, 1, None, None, None) == -1
    assert "null" in L.rs_last_error().decode()


def test_the_slot_header_kept_its_size_and_its_words(tmp_path):
    """RsGroupCell took the run's three words -- how many TTIs, where the slot's per-TTI table lies, the step between two output blocks
    -- out of its padding, behind `now`; RsLaunch is what it was: five pointers behind grp_avg."""
    src = tmp_path / "hdr.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "rs_device.h"\n'
                   'int main() { printf("%zu %d %zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(RsGroupCell), RS_GROUP_HDR_BYTES, offsetof(RsGroupCell, image_mode),\n'
                   '  offsetof(RsGroupCell, in_uid), offsetof(RsGroupCell, now), offsetof(RsGroupCell, run_ttis), offsetof(RsGroupCell, run_table),\n'
                   '  offsetof(RsGroupCell, run_out_step), sizeof(RsLaunch) - offsetof(RsLaunch, grp_avg), RS_GROUP_RUN_ROW_BYTES); return 0; }\n')
    exe = tmp_path / "hdr"
    subprocess.run(["c++", "-std=c++17", "-Wall", "-Wno-invalid-offsetof", f"-I{CSRC}", str(src), "-o", str(exe)], check=True)
    size, hdr, off_mode, off_uid, off_now, off_ttis, off_table, off_step, tail, row = (
        int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert size == hdr == 128
    assert (off_mode, off_uid, off_now) == (72, 76, 80)       # where the parent commit has them
    assert (off_ttis, off_table, off_step) == (88, 92, 96)    # the first words of what was padding
    assert tail == 5 * 8                                      # no RsLaunch field was added
    assert row == 16                                          # a table row: the clock (8 bytes), rand0, rand1
