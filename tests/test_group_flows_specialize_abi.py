"""rs_group_specialize_flows / rs_group_flows_jit_status / rs_jit_selfcheck_group_flows (not gpu): declared, exported and listed as
additions to ABI 11 (no struct moved, RsLaunch and RsGroupCell where they were); the null handle is invalid; the general and the lean
build of scheduler 1's flows kernel compile without a GPU, with the fault switch too, and every other scheduler is refused with a
message; the flows builds of a shape have cache files of their own (flag value 128 of rs_jit_cache_file / rs_jit_cache_warm, valid
only together with 8, never with 16, 32 or 64, scheduler 1 only).  Every test fails on the parent."""
import ctypes as C
import inspect
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "radiosaber_hip.h"
CSRC = ROOT / "radiosaber_amd" / "csrc"
NEW = ("rs_group_specialize_flows", "rs_group_flows_jit_status", "rs_jit_selfcheck_group_flows")
SHAPE = (1, 24, 8, 2, 256)       # one slice, 24 call positions, 8 RBGs of 2, threads: the scenario of tests/test_group_flows_abi.py
OTHER = (3, 12, 8, 2, 256)       # the other schedulers' scenario


def test_the_entry_points_are_declared_exported_and_listed(rs, tmp_path):
    txt = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    assert re.search(r"\bint\s+rs_group_specialize_flows\s*\(\s*rs_group\s*\*\s*\w+\s*\)", txt)
    assert re.search(r"\bint\s+rs_group_flows_jit_status\s*\(\s*rs_group\s*\*\s*\w+\s*,\s*char\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*\)", txt)
    assert re.search(r"\bint\s+rs_jit_selfcheck_group_flows\s*\(", txt)
    for name in NEW:
        assert hasattr(rs.lib(), name), f"{name} is declared but not exported"
        assert name in rs.api.ABI_SYMBOLS
    for attr in ("specialize_flows", "flows_jit_status"):
        assert callable(getattr(rs.GroupScheduler, attr))
    assert inspect.signature(rs.GroupScheduler.__init__).parameters["jit_flows"].default is False
    for fn in (rs.api.jit_selfcheck, rs.api.jit_cache_file, rs.api.jit_cache_warm):
        assert inspect.signature(fn).parameters["flows"].default is False
    assert rs.lib().rs_abi_version() == 11 and rs.api.RS_ABI_VERSION == 11
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "radiosaber_hip.h"\n'
                   'typedef int (*spec_fn)(rs_group*);\ntypedef int (*status_fn)(rs_group*, char*, size_t);\n'
                   'typedef int (*check_fn)(int, int, int, int, int, int, char*, size_t);\n'
                   'spec_fn f0 = rs_group_specialize_flows;\nstatus_fn f1 = rs_group_flows_jit_status;\ncheck_fn f2 = rs_jit_selfcheck_group_flows;\n'
                   'int main(void) { printf("%d %zu %zu %zu\\n", RS_ABI_VERSION, sizeof(rs_config), sizeof(rs_tti_in), sizeof(rs_tti_out));\n'
                   '  return !(f0 && f1 && f2); }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), str(rs.build.LIB), f"-Wl,-rpath,{rs.build.LIB.parent}",
                    "-o", str(exe)], check=True)
    abi, cfg, tin, tout = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert abi == 11
    assert (cfg, tin, tout) == (88, 96, 72)
    assert (cfg, tin, tout) == (C.sizeof(rs.api._Config), C.sizeof(rs.api._TtiIn), C.sizeof(rs.api._TtiOut))


def test_the_slot_header_and_the_launch_block_did_not_move(rs, tmp_path):
    """RsGroupCell and RsLaunch are untouched: the flows builds need no new word (the figures of tests/test_group_flows_abi.py)."""
    assert hasattr(rs.lib(), "rs_group_specialize_flows")
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


def test_the_null_handle_is_invalid(rs):
    L = rs.lib()
    assert L.rs_group_specialize_flows(None) == -1  # RS_ERR_INVALID
    assert "null" in L.rs_last_error().decode()
    buf = C.create_string_buffer(b"untouched", 64)
    assert L.rs_group_flows_jit_status(None, buf, 64) == -1
    assert buf.value == b"untouched"
    assert L.rs_group_flows_jit_status(None, None, 0) == -1


def test_both_flows_builds_compile(rs):
    S, U, R, G, NT = SHAPE
    buf = C.create_string_buffer(4096)
    assert rs.lib().rs_jit_selfcheck_group_flows(S, U, R, G, NT, 1, buf, 4096) > 0, buf.value.decode(errors="replace")
    assert rs.jit_selfcheck(S, U, R, G, threads=NT, sched=1, group=True, flows=True) > 0


@pytest.mark.parametrize("sched", [7, 8, 9, 10, 11, 101, 103])
def test_the_other_schedulers_have_no_flows_build(rs, sched):
    S, U, R, G, NT = OTHER
    buf = C.create_string_buffer(4096)
    assert rs.lib().rs_jit_selfcheck_group_flows(S, U, R, G, NT, sched, buf, 4096) < 0
    assert buf.value.decode(errors="replace").strip(), "refused without a message"
    with pytest.raises(rs.RadioSaberError):
        rs.jit_selfcheck(S, U, R, G, threads=NT, sched=sched, group=True, flows=True)


def test_the_fault_switch_compiles(rs, monkeypatch):
    """-DRS_FAULT_INJECT_FLOWS (tests only) takes effect under kGrpFixed && kGrpFlow: the flows builds compile with it."""
    monkeypatch.setenv("RS_JIT_EXTRA", "-DRS_FAULT_INJECT_FLOWS")
    S, U, R, G, NT = SHAPE
    assert rs.jit_selfcheck(S, U, R, G, threads=NT, sched=1, group=True, flows=True) > 0


def test_the_flows_builds_have_cache_files_of_their_own(rs, tmp_path, monkeypatch):
    monkeypatch.setenv("RS_JIT_CACHE_DIR", str(tmp_path))
    monkeypatch.delenv("RS_JIT_CACHE", raising=False)
    monkeypatch.delenv("RS_JIT_EXTRA", raising=False)
    S, U, R, G, NT = SHAPE
    L = rs.lib()
    names = []
    for flags in (1 | 8, 1 | 4 | 8, 1 | 8 | 16, 1 | 4 | 8 | 16, 1 | 8 | 128, 1 | 4 | 8 | 128):   # what scheduler 1 has: plain, resident, flows
        buf = C.create_string_buffer(4096)
        assert L.rs_jit_cache_file(S, U, R, G, NT, 1, flags, buf, 4096) > 0
        names.append(buf.value.decode())
    assert len(set(names)) == 6, names
    before = rs.jit_cache_stats()
    err = C.create_string_buffer(4096)
    assert L.rs_jit_cache_warm(S, U, R, G, NT, 1, 1 | 8 | 128, err, 4096) > 0, err.value
    assert L.rs_jit_cache_warm(S, U, R, G, NT, 1, 1 | 4 | 8 | 128, err, 4096) > 0, err.value
    files = sorted(str(f) for f in tmp_path.glob("*.rsco"))
    assert files == sorted([names[4], names[5]]), (files, names)
    after = rs.jit_cache_stats()
    assert after["misses"] - before["misses"] == 2 and after["stores"] - before["stores"] == 2
    for f in files:  # the option is part of the key text, the other forms' options are not
        text = Path(f).read_bytes()
        assert b"-DRS_JIT_GROUP=1" in text and b"-DRS_JIT_GROUP_FLOWS=1" in text
        assert b"-DRS_JIT_GROUP_QUEUED" not in text and b"-DRS_JIT_GROUP_RESIDENT" not in text and b"-DRS_JIT_GROUP_COUNTED" not in text
    assert (b"-DRS_JIT_LEAN=1" in Path(names[5]).read_bytes()) and (b"-DRS_JIT_LEAN=1" not in Path(names[4]).read_bytes())
    assert L.rs_jit_cache_warm(S, U, R, G, NT, 1, 1 | 8 | 128, err, 4096) > 0   # warming twice: one miss, then one hit
    now = rs.jit_cache_stats()
    assert now["hits"] - after["hits"] == 1 and now["misses"] == after["misses"]
    assert rs.api.jit_cache_file(S, U, R, G, NT, 1, group=True, flows=True) == names[4]
    assert rs.api.jit_cache_file(S, U, R, G, NT, 1, group=True, flows=True, lean=True) == names[5]
    assert rs.api.jit_cache_file(S, U, R, G, NT, 1, group=True) == names[0]
    assert rs.api.jit_cache_warm(S, U, R, G, NT, 1, group=True, flows=True, lean=True) > 0


def test_the_flows_flag_needs_the_group_flag_and_excludes_the_other_forms(rs, tmp_path, monkeypatch):
    monkeypatch.setenv("RS_JIT_CACHE_DIR", str(tmp_path))
    S, U, R, G, NT = SHAPE
    L = rs.lib()
    for flags in (128, 1 | 128, 1 | 4 | 128, 1 | 8 | 16 | 128, 1 | 8 | 32 | 128, 1 | 8 | 64 | 128, 1 | 8 | 32 | 64 | 128, 8 | 16 | 32 | 128):
        buf = C.create_string_buffer(b"x", 4096)
        assert L.rs_jit_cache_file(S, U, R, G, NT, 1, flags, buf, 4096) == 0 and buf.value == b"", flags
        err = C.create_string_buffer(4096)
        assert L.rs_jit_cache_warm(S, U, R, G, NT, 1, flags, err, 4096) < 0 and b"128" in err.value, (flags, err.value)
    for sched in (7, 8, 9, 10, 101, 103):   # scheduler 1 only
        err = C.create_string_buffer(4096)
        assert L.rs_jit_cache_warm(*OTHER, sched, 1 | 8 | 128, err, 4096) < 0 and b"128" in err.value and b"scheduler 1" in err.value, (sched, err.value)
    assert not list(tmp_path.glob("*.rsco"))
    with pytest.raises(ValueError):
        rs.api.jit_cache_file(S, U, R, G, NT, 1, flows=True)
    for other in ("resident", "queued", "counted"):
        with pytest.raises(ValueError):
            rs.api.jit_cache_file(S, U, R, G, NT, 1, group=True, flows=True, **{other: True})
    with pytest.raises(ValueError):
        rs.api.jit_selfcheck(S, U, R, G, threads=NT, sched=1, flows=True)
