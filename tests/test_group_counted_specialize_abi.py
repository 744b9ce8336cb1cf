"""rs_group_specialize_counted / rs_group_counted_jit_status / rs_jit_selfcheck_group_counted (not gpu): declared, exported and listed
as additions to ABI 11 (no struct moved, RsLaunch and RsGroupCell where they were); the null handle is invalid; the general and the
lean build of the counted kernel compile without a GPU for the five schedulers that have the form, with each fault switch too, and are
refused with a message for the others; the counted builds of a shape have cache files of their own (flag value 64 of rs_jit_cache_file
/ rs_jit_cache_warm, valid only together with 8 and 32), as have the flows builds (flag value 128).  Every test fails on the parent."""
import ctypes as C
import inspect
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "radiosaber_hip.h"
CSRC = ROOT / "radiosaber_amd" / "csrc"
NEW = ("rs_group_specialize_counted", "rs_group_counted_jit_status", "rs_jit_selfcheck_group_counted")
SHAPE = (3, 12, 8, 2, 256)       # slices, users, RBGs, PRBs per RBG, threads: the scenario of tests/test_group_counted_abi.py
SORT = (20, 100, 64, 8, 512)     # 1 280 sort records on 512 threads: three positions per thread
FLOWS = (1, 24, 8, 2, 256)       # scheduler 1's scenario: one slice, 24 call positions


def test_the_entry_points_are_declared_exported_and_listed(rs, tmp_path):
    txt = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    assert re.search(r"\bint\s+rs_group_specialize_counted\s*\(\s*rs_group\s*\*\s*\w+\s*\)", txt)
    assert re.search(r"\bint\s+rs_group_counted_jit_status\s*\(\s*rs_group\s*\*\s*\w+\s*,\s*char\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*\)", txt)
    assert re.search(r"\bint\s+rs_jit_selfcheck_group_counted\s*\(", txt)
    for name in NEW:
        assert hasattr(rs.lib(), name), f"{name} is declared but not exported"
        assert name in rs.api.ABI_SYMBOLS
    for attr in ("specialize_counted", "counted_jit_status"):
        assert callable(getattr(rs.GroupScheduler, attr))
    assert inspect.signature(rs.GroupScheduler.__init__).parameters["jit_counted"].default is False
    for fn in (rs.api.jit_selfcheck, rs.api.jit_cache_file, rs.api.jit_cache_warm):
        assert inspect.signature(fn).parameters["counted"].default is False
    # additions: the version and the three call structs are where they were; the probe links against the built library
    assert rs.lib().rs_abi_version() == 11 and rs.api.RS_ABI_VERSION == 11
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "radiosaber_hip.h"\n'
                   'typedef int (*spec_fn)(rs_group*);\ntypedef int (*status_fn)(rs_group*, char*, size_t);\n'
                   'typedef int (*check_fn)(int, int, int, int, int, int, char*, size_t);\n'
                   'spec_fn f0 = rs_group_specialize_counted;\nstatus_fn f1 = rs_group_counted_jit_status;\ncheck_fn f2 = rs_jit_selfcheck_group_counted;\n'
                   'int main(void) { printf("%d %zu %zu %zu\\n", RS_ABI_VERSION, sizeof(rs_config), sizeof(rs_tti_in), sizeof(rs_tti_out));\n'
                   '  return !(f0 && f1 && f2); }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), str(rs.build.LIB), f"-Wl,-rpath,{rs.build.LIB.parent}",
                    "-o", str(exe)], check=True)
    abi, cfg, tin, tout = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert abi == 11
    assert (cfg, tin, tout) == (88, 96, 72)
    assert (cfg, tin, tout) == (C.sizeof(rs.api._Config), C.sizeof(rs.api._TtiIn), C.sizeof(rs.api._TtiOut))


def test_the_slot_header_and_the_group_fields_kept_their_places(rs, tmp_path):
    """RsGroupCell and RsLaunch are untouched: the counted builds need no new word (the figures of tests/test_group_counted_abi.py)."""
    assert hasattr(rs.lib(), "rs_group_specialize_counted")
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
    assert L.rs_group_specialize_counted(None) == -1  # RS_ERR_INVALID
    assert "null" in L.rs_last_error().decode()
    buf = C.create_string_buffer(b"untouched", 64)
    assert L.rs_group_counted_jit_status(None, buf, 64) == -1
    assert buf.value == b"untouched"
    assert L.rs_group_counted_jit_status(None, None, 0) == -1


@pytest.mark.parametrize("sched", [7, 8, 9, 101, 103])
def test_both_counted_builds_compile(rs, sched):
    S, U, R, G, NT = SHAPE
    buf = C.create_string_buffer(4096)
    assert rs.lib().rs_jit_selfcheck_group_counted(S, U, R, G, NT, sched, buf, 4096) > 0, buf.value.decode(errors="replace")
    assert rs.jit_selfcheck(S, U, R, G, threads=NT, sched=sched, group=True, counted=True) > 0


def test_both_counted_builds_compile_at_the_sort_shape(rs):
    S, U, R, G, NT = SORT
    assert rs.jit_selfcheck(S, U, R, G, threads=NT, sched=9, group=True, counted=True) > 0


@pytest.mark.parametrize("sched", [1, 10, 11])
def test_the_other_schedulers_have_no_counted_build(rs, sched):
    S, U, R, G, NT = SHAPE
    buf = C.create_string_buffer(4096)
    assert rs.lib().rs_jit_selfcheck_group_counted(S, U, R, G, NT, sched, buf, 4096) < 0
    assert buf.value.decode(errors="replace").strip(), "refused without a message"
    with pytest.raises(rs.RadioSaberError):
        rs.jit_selfcheck(S, U, R, G, threads=NT, sched=sched, group=True, counted=True)
    assert rs.lib().rs_jit_selfcheck_group_queued(S, U, R, G, NT, 1, buf, 4096) < 0   # (as before: scheduler 1 has no queued build)


@pytest.mark.parametrize("switch", ["-DRS_FAULT_INJECT_COUNTED=1", "-DRS_FAULT_INJECT_COUNTED=2"])
def test_the_fault_switches_compile(rs, monkeypatch, switch):
    """tests only: they take effect under kGrpFixed && kGrpCnt, and the counted builds compile with each"""
    monkeypatch.setenv("RS_JIT_EXTRA", switch)
    S, U, R, G, NT = SHAPE
    assert rs.jit_selfcheck(S, U, R, G, threads=NT, sched=9, group=True, counted=True) > 0


# general and lean build of the five forms of a group's kernel: plain, resident, queued, counted, flows
TEN = (1 | 8, 1 | 4 | 8, 1 | 8 | 16, 1 | 4 | 8 | 16, 1 | 8 | 32, 1 | 4 | 8 | 32, 1 | 8 | 32 | 64, 1 | 4 | 8 | 32 | 64, 1 | 8 | 128, 1 | 4 | 8 | 128)


def test_the_counted_builds_have_cache_files_of_their_own(rs, tmp_path, monkeypatch):
    monkeypatch.setenv("RS_JIT_CACHE_DIR", str(tmp_path))
    monkeypatch.delenv("RS_JIT_CACHE", raising=False)
    monkeypatch.delenv("RS_JIT_EXTRA", raising=False)
    S, U, R, G, NT = SHAPE
    L = rs.lib()
    names = []
    for flags in TEN:
        buf = C.create_string_buffer(4096)
        shape, sched = (FLOWS, 1) if flags & 128 else (SHAPE, 9)
        assert L.rs_jit_cache_file(*shape, sched, flags, buf, 4096) > 0, flags
        names.append(buf.value.decode())
    assert len(set(names)) == 10, names
    # ... and at ONE shape and scheduler, the eight combinations that scheduler 9 has
    same = []
    for flags in TEN[:8]:
        buf = C.create_string_buffer(4096)
        assert L.rs_jit_cache_file(S, U, R, G, NT, 9, flags, buf, 4096) > 0
        same.append(buf.value.decode())
    assert len(set(same)) == 8
    before = rs.jit_cache_stats()
    err = C.create_string_buffer(4096)
    assert L.rs_jit_cache_warm(S, U, R, G, NT, 9, 1 | 8 | 32 | 64, err, 4096) > 0, err.value
    assert L.rs_jit_cache_warm(S, U, R, G, NT, 9, 1 | 4 | 8 | 32 | 64, err, 4096) > 0, err.value
    files = sorted(str(f) for f in tmp_path.glob("*.rsco"))
    assert files == sorted([names[6], names[7]]), (files, names)
    after = rs.jit_cache_stats()
    assert after["misses"] - before["misses"] == 2 and after["stores"] - before["stores"] == 2
    for f in files:  # the option is part of the key text, the other forms' options are not
        text = Path(f).read_bytes()
        assert b"-DRS_JIT_GROUP=1" in text and b"-DRS_JIT_GROUP_COUNTED=1" in text
        assert b"-DRS_JIT_GROUP_QUEUED" not in text and b"-DRS_JIT_GROUP_RESIDENT" not in text and b"-DRS_JIT_GROUP_FLOWS" not in text
    assert (b"-DRS_JIT_LEAN=1" in Path(names[7]).read_bytes()) and (b"-DRS_JIT_LEAN=1" not in Path(names[6]).read_bytes())
    assert L.rs_jit_cache_warm(S, U, R, G, NT, 9, 1 | 8 | 32 | 64, err, 4096) > 0   # warming twice: one miss, then one hit
    now = rs.jit_cache_stats()
    assert now["hits"] - after["hits"] == 1 and now["misses"] == after["misses"]
    assert rs.api.jit_cache_file(S, U, R, G, NT, 9, group=True, counted=True) == names[6]
    assert rs.api.jit_cache_file(S, U, R, G, NT, 9, group=True, counted=True, lean=True) == names[7]
    assert rs.api.jit_cache_file(S, U, R, G, NT, 9, group=True, queued=True) == names[4]
    assert rs.api.jit_cache_warm(S, U, R, G, NT, 9, group=True, counted=True, lean=True) > 0


def test_the_counted_flag_needs_the_group_flag_and_the_queued_flag(rs, tmp_path, monkeypatch):
    monkeypatch.setenv("RS_JIT_CACHE_DIR", str(tmp_path))
    S, U, R, G, NT = SHAPE
    L = rs.lib()
    for flags in (64, 1 | 64, 1 | 8 | 64, 1 | 32 | 64, 1 | 4 | 8 | 64, 8 | 16 | 64):   # 64 without 8 or without 32
        buf = C.create_string_buffer(b"x", 4096)
        assert L.rs_jit_cache_file(S, U, R, G, NT, 9, flags, buf, 4096) == 0 and buf.value == b"", flags
        err = C.create_string_buffer(4096)
        assert L.rs_jit_cache_warm(S, U, R, G, NT, 9, flags, err, 4096) < 0 and b"64" in err.value, (flags, err.value)
    err = C.create_string_buffer(4096)
    assert L.rs_jit_cache_warm(S, U, R, G, NT, 9, 1 | 8 | 16 | 32 | 64, err, 4096) < 0 and err.value   # (the queued flag's own rule)
    assert L.rs_jit_cache_warm(S, U, R, G, NT, 10, 1 | 8 | 32 | 64, err, 4096) < 0 and b"7, 8, 9, 101 and 103" in err.value  # no counted form
    assert not list(tmp_path.glob("*.rsco"))
    # the answers of the combinations that existed before are what they were
    assert L.rs_jit_cache_warm(S, U, R, G, NT, 9, 1 | 8 | 16 | 32, err, 4096) < 0
    assert err.value == b"flag values 16 (the resident form) and 32 (the queued form) exclude each other"
    assert L.rs_jit_cache_warm(S, U, R, G, NT, 9, 1 | 32, err, 4096) < 0
    assert err.value == b"flag value 32 (the queued form) is valid only together with 8 (a group's build)"
    with pytest.raises(ValueError):
        rs.api.jit_cache_file(S, U, R, G, NT, 9, counted=True)
    with pytest.raises(ValueError):
        rs.api.jit_cache_file(S, U, R, G, NT, 9, group=True, resident=True, counted=True)
    with pytest.raises(ValueError):
        rs.api.jit_cache_warm(S, U, R, G, NT, 9, group=True, counted=True, flows=True)
    with pytest.raises(ValueError):
        rs.api.jit_selfcheck(S, U, R, G, threads=NT, sched=9, counted=True)
