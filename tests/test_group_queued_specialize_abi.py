"""rs_group_specialize_queued / rs_group_queued_jit_status / rs_jit_selfcheck_group_queued (not gpu): declared, exported and listed as
additions to ABI 11 (no struct moved, RsLaunch and RsGroupCell where they were); the null handle is invalid; the general and the lean
build of the queued kernel compile without a GPU for the five schedulers that have a queued form and are refused with a message for
the others; the queued builds of a shape have cache files of their own (flag value 32 of rs_jit_cache_file / rs_jit_cache_warm, valid
only together with 8 and never together with 16)."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "radiosaber_hip.h"
CSRC = ROOT / "radiosaber_amd" / "csrc"
NEW = ("rs_group_specialize_queued", "rs_group_queued_jit_status", "rs_jit_selfcheck_group_queued")
SHAPE = (3, 12, 8, 2, 256)       # slices, users, RBGs, PRBs per RBG, threads: the scenario of tests/test_group_queued_abi.py
SORT = (20, 100, 64, 8, 512)     # 1 280 sort records on 512 threads: three positions per thread


def test_the_entry_points_are_declared_exported_and_listed(rs, tmp_path):
    txt = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    assert re.search(r"\bint\s+rs_group_specialize_queued\s*\(\s*rs_group\s*\*\s*\w+\s*\)", txt)
    assert re.search(r"\bint\s+rs_group_queued_jit_status\s*\(\s*rs_group\s*\*\s*\w+\s*,\s*char\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*\)", txt)
    assert re.search(r"\bint\s+rs_jit_selfcheck_group_queued\s*\(", txt)
    for name in NEW:
        assert hasattr(rs.lib(), name), f"{name} is declared but not exported"
        assert name in rs.api.ABI_SYMBOLS
    for attr in ("specialize_queued", "queued_jit_status"):
        assert callable(getattr(rs.GroupScheduler, attr))
    import inspect
    assert inspect.signature(rs.GroupScheduler.__init__).parameters["jit_queued"].default is False
    # additions: the version and the three call structs are where they were; the probe links against the built library
    assert rs.lib().rs_abi_version() == 11 and rs.api.RS_ABI_VERSION == 11
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "radiosaber_hip.h"\n'
                   'typedef int (*spec_fn)(rs_group*);\ntypedef int (*status_fn)(rs_group*, char*, size_t);\n'
                   'typedef int (*check_fn)(int, int, int, int, int, int, char*, size_t);\n'
                   'spec_fn f0 = rs_group_specialize_queued;\nstatus_fn f1 = rs_group_queued_jit_status;\ncheck_fn f2 = rs_jit_selfcheck_group_queued;\n'
                   'int main(void) { printf("%d %zu %zu %zu\\n", RS_ABI_VERSION, sizeof(rs_config), sizeof(rs_tti_in), sizeof(rs_tti_out));\n'
                   '  return !(f0 && f1 && f2); }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), str(rs.build.LIB), f"-Wl,-rpath,{rs.build.LIB.parent}",
                    "-o", str(exe)], check=True)
    abi, cfg, tin, tout = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert abi == 11
    assert (cfg, tin, tout) == (88, 96, 72)
    assert (cfg, tin, tout) == (C.sizeof(rs.api._Config), C.sizeof(rs.api._TtiIn), C.sizeof(rs.api._TtiOut))


def test_the_slot_header_and_the_group_fields_kept_their_places(tmp_path):
    """RsGroupCell and RsLaunch are untouched: the queued builds need no new word (the figures of tests/test_group_queued_abi.py)."""
    src = tmp_path / "hdr.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "rs_device.h"\n'
                   'int main() { printf("%zu %d %zu %zu %zu %zu\\n", sizeof(RsGroupCell), RS_GROUP_HDR_BYTES, offsetof(RsGroupCell, in_uid),\n'
                   '  offsetof(RsGroupCell, now), offsetof(RsLaunch, grp_in) - offsetof(RsLaunch, grp_qavg),\n'
                   '  sizeof(RsLaunch) - offsetof(RsLaunch, grp_avg)); return 0; }\n')
    exe = tmp_path / "hdr"
    subprocess.run(["c++", "-std=c++17", "-Wall", "-Wno-invalid-offsetof", f"-I{CSRC}", str(src), "-o", str(exe)], check=True)
    size, hdr, off_uid, off_now, block, tail = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert size == hdr == 128 and (off_uid, off_now) == (76, 80)
    assert block == 6 * 8 and tail == 5 * 8


def test_the_null_handle_is_invalid(rs):
    L = rs.lib()
    assert L.rs_group_specialize_queued(None) == -1  # RS_ERR_INVALID
    assert "null" in L.rs_last_error().decode()
    buf = C.create_string_buffer(b"untouched", 64)
    assert L.rs_group_queued_jit_status(None, buf, 64) == -1
    assert buf.value == b"untouched"
    assert L.rs_group_queued_jit_status(None, None, 0) == -1


@pytest.mark.parametrize("sched", [7, 8, 9, 101, 103])
def test_both_queued_builds_compile(rs, sched):
    S, U, R, G, NT = SHAPE
    buf = C.create_string_buffer(4096)
    assert rs.lib().rs_jit_selfcheck_group_queued(S, U, R, G, NT, sched, buf, 4096) > 0, buf.value.decode(errors="replace")
    assert rs.jit_selfcheck(S, U, R, G, threads=NT, sched=sched, group=True, queued=True) > 0


def test_both_queued_builds_compile_at_the_sort_shape(rs):
    S, U, R, G, NT = SORT
    assert rs.jit_selfcheck(S, U, R, G, threads=NT, sched=9, group=True, queued=True) > 0


@pytest.mark.parametrize("sched", [1, 10, 11])
def test_the_other_schedulers_have_no_queued_build(rs, sched):
    S, U, R, G, NT = SHAPE
    buf = C.create_string_buffer(4096)
    assert rs.lib().rs_jit_selfcheck_group_queued(S, U, R, G, NT, sched, buf, 4096) < 0
    assert buf.value.decode(errors="replace").strip(), "refused without a message"
    with pytest.raises(rs.RadioSaberError):
        rs.jit_selfcheck(S, U, R, G, threads=NT, sched=sched, group=True, queued=True)


def test_the_fault_switch_compiles_and_changes_the_queued_builds_only(rs, monkeypatch):
    """-DRS_FAULT_INJECT_QUEUED (tests only) takes effect under kGrpFixed && kGrpQue: the queued builds compile with it."""
    monkeypatch.setenv("RS_JIT_EXTRA", "-DRS_FAULT_INJECT_QUEUED")
    S, U, R, G, NT = SHAPE
    assert rs.jit_selfcheck(S, U, R, G, threads=NT, sched=9, group=True, queued=True) > 0


def test_the_queued_builds_have_cache_files_of_their_own(rs, tmp_path, monkeypatch):
    monkeypatch.setenv("RS_JIT_CACHE_DIR", str(tmp_path))
    monkeypatch.delenv("RS_JIT_CACHE", raising=False)
    monkeypatch.delenv("RS_JIT_EXTRA", raising=False)
    S, U, R, G, NT = SHAPE
    L = rs.lib()
    names = []
    for flags in (1 | 8, 1 | 8 | 16, 1 | 8 | 32, 1 | 4 | 8 | 32, 1 | 4 | 8, 1 | 4 | 8 | 16):
        buf = C.create_string_buffer(4096)
        assert L.rs_jit_cache_file(S, U, R, G, NT, 9, flags, buf, 4096) > 0
        names.append(buf.value.decode())
    assert len(set(names)) == 6, names
    before = rs.jit_cache_stats()
    err = C.create_string_buffer(4096)
    assert L.rs_jit_cache_warm(S, U, R, G, NT, 9, 1 | 8 | 32, err, 4096) > 0, err.value
    assert L.rs_jit_cache_warm(S, U, R, G, NT, 9, 1 | 4 | 8 | 32, err, 4096) > 0, err.value
    files = sorted(str(f) for f in tmp_path.glob("*.rsco"))
    assert files == sorted([names[2], names[3]]), (files, names)
    after = rs.jit_cache_stats()
    assert after["misses"] - before["misses"] == 2 and after["stores"] - before["stores"] == 2
    for f in files:  # the option is part of the key text
        text = Path(f).read_bytes()
        assert b"-DRS_JIT_GROUP=1" in text and b"-DRS_JIT_GROUP_QUEUED=1" in text and b"-DRS_JIT_GROUP_RESIDENT" not in text
    assert (b"-DRS_JIT_LEAN=1" in Path(names[3]).read_bytes()) and (b"-DRS_JIT_LEAN=1" not in Path(names[2]).read_bytes())
    assert L.rs_jit_cache_warm(S, U, R, G, NT, 9, 1 | 8 | 32, err, 4096) > 0
    assert rs.jit_cache_stats()["hits"] - after["hits"] == 1
    assert rs.api.jit_cache_file(S, U, R, G, NT, 9, group=True, queued=True) == names[2]
    assert rs.api.jit_cache_file(S, U, R, G, NT, 9, group=True, queued=True, lean=True) == names[3]
    assert rs.api.jit_cache_file(S, U, R, G, NT, 9, group=True) == names[0]
    assert rs.api.jit_cache_warm(S, U, R, G, NT, 9, group=True, queued=True, lean=True) > 0


def test_the_queued_flag_needs_the_group_flag_and_excludes_the_resident_flag(rs, tmp_path, monkeypatch):
    monkeypatch.setenv("RS_JIT_CACHE_DIR", str(tmp_path))
    S, U, R, G, NT = SHAPE
    L = rs.lib()
    for flags in (1 | 32, 32, 1 | 4 | 32, 1 | 8 | 16 | 32, 8 | 16 | 32):
        buf = C.create_string_buffer(b"x", 4096)
        assert L.rs_jit_cache_file(S, U, R, G, NT, 9, flags, buf, 4096) == 0 and buf.value == b"", flags
        err = C.create_string_buffer(4096)
        assert L.rs_jit_cache_warm(S, U, R, G, NT, 9, flags, err, 4096) < 0 and b"32" in err.value, (flags, err.value)
    err = C.create_string_buffer(4096)
    assert L.rs_jit_cache_warm(S, U, R, G, NT, 10, 1 | 8 | 32, err, 4096) < 0 and b"7, 8, 9, 101 and 103" in err.value  # no queued form
    assert not list(tmp_path.glob("*.rsco"))
    with pytest.raises(ValueError):
        rs.api.jit_cache_file(S, U, R, G, NT, 9, queued=True)
    with pytest.raises(ValueError):
        rs.api.jit_cache_file(S, U, R, G, NT, 9, group=True, resident=True, queued=True)
