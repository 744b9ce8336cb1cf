"""rs_group_image_stats and the per-slot image mode of a group call (not gpu): the entry point is declared, exported and listed; it is
an addition to ABI 11 -- no struct moved -- and the slot header of the group kernels kept its size."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "radiosaber_hip.h"
CSRC = ROOT / "radiosaber_amd" / "csrc"


def test_image_stats_is_declared_exported_and_listed(rs):
    txt = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    assert re.search(r"\bint\s+rs_group_image_stats\s*\(\s*const\s+rs_group\s*\*\s*\w+\s*,\s*int64_t\s+\w+\[3\]\s*\)", txt)
    assert hasattr(rs.lib(), "rs_group_image_stats"), "declared but not exported"
    assert "rs_group_image_stats" in rs.api.ABI_SYMBOLS
    assert isinstance(rs.GroupScheduler.image_stats, property)
    assert "accepted and ignored" not in HEADER.read_text()  # the group rule that this entry point replaces


def test_null_arguments_are_invalid(rs):
    out = np.full(3, -7, np.int64)
    assert rs.lib().rs_group_image_stats(None, out.ctypes.data_as(C.POINTER(C.c_int64))) == -1
    assert "null" in rs.lib().rs_last_error().decode()
    assert rs.lib().rs_group_image_stats(None, None) == -1
    assert out.tolist() == [-7, -7, -7]


def test_abi_version_and_struct_sizes_did_not_move(rs, tmp_path):
    assert rs.lib().rs_abi_version() == 11 and rs.api.RS_ABI_VERSION == 11
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "radiosaber_hip.h"\n'
                   'typedef int (*stats_fn)(const rs_group*, int64_t*);\n'
                   'enum { declared = sizeof((stats_fn)rs_group_image_stats) }; /* (the prototype is what this line checks) */\n'
                   'int main(void) { printf("%d %zu %zu %zu\\n", RS_ABI_VERSION, sizeof(rs_config), sizeof(rs_tti_in), sizeof(rs_tti_out)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    abi, cfg, tin, tout = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert abi == 11
    assert (cfg, tin, tout) == (88, 96, 72)
    assert (cfg, tin, tout) == (C.sizeof(rs.api._Config), C.sizeof(rs.api._TtiIn), C.sizeof(rs.api._TtiOut))


def test_the_slot_header_kept_its_size(tmp_path):
    """RsGroupCell got its image_mode word out of its padding: a compiled probe of the device header (host compiler; the header's own
    static_assert says the same to every build of the library)."""
    assert re.search(r"static_assert\(sizeof\(RsGroupCell\) == RS_GROUP_HDR_BYTES", (CSRC / "rs_device.h").read_text())
    src = tmp_path / "hdr.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "rs_device.h"\n'
                   'int main() { printf("%zu %d %zu %zu %zu\\n", sizeof(RsGroupCell), RS_GROUP_HDR_BYTES, offsetof(RsGroupCell, image_mode),\n'
                   '  offsetof(RsGroupCell, out_upper), offsetof(RsLaunch, grp_image) - offsetof(RsLaunch, grp_count)); return 0; }\n')
    exe = tmp_path / "hdr"
    subprocess.run(["c++", "-std=c++17", "-Wall", "-Wno-invalid-offsetof", f"-I{CSRC}", str(src), "-o", str(exe)], check=True)
    size, hdr, off_mode, off_upper, gap = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert size == hdr == 128
    assert off_mode == off_upper + 4   # the first word of what was padding: the words before it did not move
    assert gap == 8                     # the stores are appended behind what was RsLaunch's last field
