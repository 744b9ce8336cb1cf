"""Resident averages of a group's cells (not gpu): rs_group_set_avg / rs_group_get_avg / rs_group_set_pending /
rs_group_schedule_tti_at are declared, exported and listed; they are additions to ABI 11 -- no struct moved -- and the slot header of
the group kernels took its two new words out of its padding."""
import ctypes as C
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "radiosaber_amd" / "csrc"
NEW = ("rs_group_set_avg", "rs_group_get_avg", "rs_group_set_pending", "rs_group_schedule_tti_at")


def test_the_four_prototypes_compile_and_nothing_moved(rs, tmp_path):
    """A C probe against the public header: assigning each entry point to a pointer of the documented type is what checks the
    prototype (-Werror: an incompatible pointer type stops the build); then the version and the three struct sizes."""
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "radiosaber_hip.h"\n'
                   'typedef int (*set_avg_fn)(rs_group*, int32_t, const double*, double);\n'
                   'typedef int (*get_avg_fn)(rs_group*, int32_t, double*, int32_t*, double*);\n'
                   'typedef int (*set_pending_fn)(rs_group*, int32_t, const int32_t*);\n'
                   'typedef int (*tti_at_fn)(rs_group*, int32_t, const int32_t*, const rs_tti_in*, rs_tti_out*, const double*);\n'
                   'set_avg_fn f0 = rs_group_set_avg;\nget_avg_fn f1 = rs_group_get_avg;\n'
                   'set_pending_fn f2 = rs_group_set_pending;\ntti_at_fn f3 = rs_group_schedule_tti_at;\n'
                   'int main(void) { printf("%d %zu %zu %zu\\n", RS_ABI_VERSION, sizeof(rs_config), sizeof(rs_tti_in), sizeof(rs_tti_out));\n'
                   '  return !(f0 && f1 && f2 && f3); }\n')
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
    for method in ("set_avg", "get_avg", "set_pending", "schedule_tti_at"):
        assert callable(getattr(rs.GroupScheduler, method))


def test_null_arguments_are_invalid(rs):
    L = rs.lib()
    assert L.rs_group_set_avg(None, 0, None, 0.0) == -1
    assert L.rs_group_get_avg(None, 0, None, None, None) == -1
    assert L.rs_group_set_pending(None, 0, None) == -1
    assert L.rs_group_schedule_tti_at(None, 1, None, None, None, None) == -1
    assert "null" in L.rs_last_error().decode()


def test_the_slot_header_kept_its_size_and_its_words(tmp_path):
    """RsGroupCell took the slot's clock and the offset of its user-id list out of its padding; RsLaunch grew behind its last field."""
    src = tmp_path / "hdr.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "rs_device.h"\n'
                   'int main() { printf("%zu %d %zu %zu %zu %zu %zu %zu\\n", sizeof(RsGroupCell), RS_GROUP_HDR_BYTES, offsetof(RsGroupCell, image_mode),\n'
                   '  offsetof(RsGroupCell, out_upper), offsetof(RsGroupCell, in_uid), offsetof(RsGroupCell, now),\n'
                   '  offsetof(RsLaunch, grp_avg) - offsetof(RsLaunch, grp_prb_stride), sizeof(RsLaunch) - offsetof(RsLaunch, grp_avg)); return 0; }\n')
    exe = tmp_path / "hdr"
    subprocess.run(["c++", "-std=c++17", "-Wall", "-Wno-invalid-offsetof", f"-I{CSRC}", str(src), "-o", str(exe)], check=True)
    size, hdr, off_mode, off_upper, off_uid, off_now, gap, tail = (
        int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert size == hdr == 128
    assert off_mode == 72 == off_upper + 4     # where the parent commit has it: 18 words before it
    assert (off_uid, off_now) == (76, 80)      # the first words of what was padding
    assert gap == 8 and tail == 5 * 8          # five pointers appended behind what was RsLaunch's last field

