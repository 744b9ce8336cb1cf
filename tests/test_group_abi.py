"""The group entry points of the C ABI (not gpu): rs_group_* are declared, exported and additive -- the ABI version and the three
call structs keep their layout -- and, like every compute entry point, they refuse to work without a device."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "radiosaber_hip.h"
GROUP_ENTRY_POINTS = ("rs_group_create", "rs_group_destroy", "rs_group_schedule_tti", "rs_group_get_slice_offset",
                      "rs_group_set_slice_offset", "rs_group_launch_count", "rs_group_kernel_name")


def test_header_declares_the_group_entry_points_and_the_library_exports_them(rs):
    txt = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    L = rs.lib()
    for name in GROUP_ENTRY_POINTS + ("rs_group_create_checked",):
        assert re.search(r"\b%s\s*\(" % name, txt), f"{name} is not declared in include/radiosaber_hip.h"
        assert hasattr(L, name), f"{name} is declared but not exported"
        assert name in rs.api.ABI_SYMBOLS
    assert re.search(r"#define\s+RS_GROUP_CREATE\(", txt)
    assert re.search(r"#define\s+RS_GROUP_MAX_CELLS\s+1024\b", txt)
    assert hasattr(rs, "GroupScheduler")


def test_the_group_call_is_an_addition_to_abi_11(rs, tmp_path):
    """rs_abi_version() stays 11 and sizeof(rs_config / rs_tti_in / rs_tti_out) is what the ctypes mirrors say (no field added)."""
    assert rs.lib().rs_abi_version() == 11 and rs.api.RS_ABI_VERSION == 11
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "radiosaber_hip.h"\n'
                   'int main(void) { printf("%d %zu %zu %zu %d\\n", RS_ABI_VERSION, sizeof(rs_config), sizeof(rs_tti_in), sizeof(rs_tti_out), '
                   'RS_GROUP_MAX_CELLS); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    abi, cfg, tin, tout, max_cells = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert abi == 11 and max_cells == 1024
    assert cfg == C.sizeof(rs.api._Config)
    assert tin == C.sizeof(rs.api._TtiIn)
    assert tout == C.sizeof(rs.api._TtiOut)
    # the values the parent commit's header gave (LP64): an added field would move them
    assert (cfg, tin, tout) == (88, 96, 72)


def test_group_create_validates_before_it_looks_for_a_device(rs):
    """A bad n_cells, scheduler 11 and a stale ABI are RS_ERR_INVALID with a message -- with or without a GPU."""
    L = rs.lib()
    sc = rs.SliceConfig([2, 2])
    for n_cells in (0, -3, 1025):
        with pytest.raises(rs.RadioSaberError) as e:
            rs.GroupScheduler(sc, 12, 2, n_cells)
        assert "n_cells" in str(e.value) and "1..1024" in str(e.value)
    with pytest.raises(rs.RadioSaberError) as e:
        rs.GroupScheduler(sc, 12, 2, 4, sched=rs.RS_SCHED_NVS_NONGREEDY)
    assert "RS_SCHED_NVS_NONGREEDY" in str(e.value)
    holder = rs.api._CfgHolder(sc, 12, 2, rs.RS_SCHED_MAXCELL, 0, None)
    assert not L.rs_group_create_checked(C.byref(holder.c), 4, 10, C.sizeof(rs.api._Config))
    assert "ABI mismatch" in L.rs_last_error().decode()
    assert not L.rs_group_create_checked(C.byref(holder.c), 4, 11, C.sizeof(rs.api._Config) + 8)
    assert "ABI mismatch" in L.rs_last_error().decode()
    assert not L.rs_group_create(None, 4)
    # the null handle is harmless everywhere
    L.rs_group_destroy(None)
    assert L.rs_group_launch_count(None) == 0
    assert L.rs_group_schedule_tti(None, 1, None, None, None) == -1


def test_no_cpu_fallback_for_groups(rs):
    if rs.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(rs.RadioSaberError) as e:
        rs.GroupScheduler(rs.SliceConfig([2, 2]), 12, 2, 4)
    assert "no HIP device" in str(e.value)
