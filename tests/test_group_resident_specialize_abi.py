"""rs_group_specialize_resident / rs_group_resident_jit_status / rs_jit_selfcheck_group_resident (not gpu): declared, exported and listed
as additions to ABI 11 (no struct moved); the null handle is invalid; the general and the lean build of the resident kernel compile
without a GPU for every scheduler a group serves, and not for scheduler 11; the four group builds of one shape -- plain and resident,
general and lean -- never share a cache file (flag value 16 of rs_jit_cache_file / rs_jit_cache_warm, valid only together with 8)."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "radiosaber_hip.h"
NEW = ("rs_group_specialize_resident", "rs_group_resident_jit_status", "rs_jit_selfcheck_group_resident")
SMALL = (5, 14, 12, 2, 256)      # slices, users, RBGs, PRBs per RBG, threads: the small shape of tests/test_group_specialize_abi.py
SORT = (20, 100, 64, 8, 512)     # 1 280 sort records on 512 threads: three positions per thread


def test_the_entry_points_are_declared_exported_and_listed(rs, tmp_path):
    txt = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    assert re.search(r"\bint\s+rs_group_specialize_resident\s*\(\s*rs_group\s*\*\s*\w+\s*\)", txt)
    assert re.search(r"\bint\s+rs_group_resident_jit_status\s*\(\s*rs_group\s*\*\s*\w+\s*,\s*char\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*\)", txt)
    assert re.search(r"\bint\s+rs_jit_selfcheck_group_resident\s*\(", txt)
    for name in NEW:
        assert hasattr(rs.lib(), name), f"{name} is declared but not exported"
        assert name in rs.api.ABI_SYMBOLS
    for attr in ("specialize_resident", "resident_jit_status"):
        assert callable(getattr(rs.GroupScheduler, attr))
    # additions: the version and the three call structs are where they were
    assert rs.lib().rs_abi_version() == 11 and rs.api.RS_ABI_VERSION == 11
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "radiosaber_hip.h"\n'
                   'typedef int (*spec_fn)(rs_group*);\ntypedef int (*status_fn)(rs_group*, char*, size_t);\n'
                   'typedef int (*check_fn)(int, int, int, int, int, int, char*, size_t);\n'
                   'enum { declared = sizeof((spec_fn)rs_group_specialize_resident) + sizeof((status_fn)rs_group_resident_jit_status) + '
                   'sizeof((check_fn)rs_jit_selfcheck_group_resident) }; /* (the prototypes are what this line checks) */\n'
                   'int main(void) { printf("%d %zu %zu %zu\\n", RS_ABI_VERSION, sizeof(rs_config), sizeof(rs_tti_in), sizeof(rs_tti_out)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    abi, cfg, tin, tout = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert abi == 11
    assert (cfg, tin, tout) == (88, 96, 72)
    assert (cfg, tin, tout) == (C.sizeof(rs.api._Config), C.sizeof(rs.api._TtiIn), C.sizeof(rs.api._TtiOut))


def test_the_null_handle_is_invalid(rs):
    L = rs.lib()
    assert L.rs_group_specialize_resident(None) == -1  # RS_ERR_INVALID
    assert "null" in L.rs_last_error().decode()
    buf = C.create_string_buffer(b"untouched", 64)
    assert L.rs_group_resident_jit_status(None, buf, 64) == -1
    assert buf.value == b"untouched"
    assert L.rs_group_resident_jit_status(None, None, 0) == -1


@pytest.mark.parametrize("sched", [1, 7, 8, 9, 10, 101, 103])
def test_both_resident_builds_compile_at_the_small_shape(rs, sched):
    S, U, R, G, NT = SMALL
    assert rs.jit_selfcheck(S, U, R, G, threads=NT, sched=sched, group=True, resident=True) > 0


def test_both_resident_builds_compile_at_the_sort_shape(rs):
    S, U, R, G, NT = SORT
    assert rs.jit_selfcheck(S, U, R, G, threads=NT, sched=9, group=True, resident=True) > 0


def test_scheduler_11_has_no_resident_build(rs):
    S, U, R, G, NT = SMALL
    buf = C.create_string_buffer(4096)
    assert rs.lib().rs_jit_selfcheck_group_resident(S, U, R, G, NT, 11, buf, 4096) < 0
    log = buf.value.decode(errors="replace")
    assert log.strip() and "group calls" in log, log  # the static_assert of the cell body
    with pytest.raises(rs.RadioSaberError):
        rs.jit_selfcheck(S, U, R, G, threads=NT, sched=11, group=True, resident=True)


def test_the_four_group_builds_never_share_a_cache_file(rs, tmp_path, monkeypatch):
    monkeypatch.setenv("RS_JIT_CACHE_DIR", str(tmp_path))
    monkeypatch.delenv("RS_JIT_CACHE", raising=False)
    monkeypatch.delenv("RS_JIT_EXTRA", raising=False)
    S, U, R, G, NT = SMALL
    L = rs.lib()
    names = []
    for flags in (1 | 8, 1 | 4 | 8, 1 | 8 | 16, 1 | 4 | 8 | 16):  # the plain and the resident group kernel, general and lean
        buf = C.create_string_buffer(4096)
        assert L.rs_jit_cache_file(S, U, R, G, NT, 8, flags, buf, 4096) > 0
        names.append(buf.value.decode())
    assert len(set(names)) == 4, names
    before = rs.jit_cache_stats()
    err = C.create_string_buffer(4096)
    assert L.rs_jit_cache_warm(S, U, R, G, NT, 8, 1 | 8, err, 4096) > 0, err.value
    assert L.rs_jit_cache_warm(S, U, R, G, NT, 8, 1 | 8 | 16, err, 4096) > 0, err.value
    files = sorted(str(f) for f in tmp_path.glob("*.rsco"))
    assert files == sorted([names[0], names[2]]), (files, names)
    after = rs.jit_cache_stats()
    assert after["misses"] - before["misses"] == 2 and after["stores"] - before["stores"] == 2
    # the key text in the file says which is which
    texts = {f: Path(f).read_bytes() for f in files}
    assert b"-DRS_JIT_GROUP_RESIDENT=1" in texts[names[2]] and b"-DRS_JIT_GROUP_RESIDENT=1" not in texts[names[0]]
    assert b"-DRS_JIT_GROUP=1" in texts[names[0]] and b"-DRS_JIT_GROUP=1" in texts[names[2]]
    # and each is found again under its own key
    for n, flags in enumerate((1 | 8, 1 | 8 | 16)):
        assert L.rs_jit_cache_warm(S, U, R, G, NT, 8, flags, err, 4096) > 0
        assert rs.jit_cache_stats()["hits"] - after["hits"] == n + 1
    assert sorted(str(f) for f in tmp_path.glob("*.rsco")) == files
    assert rs.api.jit_cache_file(S, U, R, G, NT, 8, group=True, resident=True) == names[2]
    assert rs.api.jit_cache_file(S, U, R, G, NT, 8, group=True, resident=True, lean=True) == names[3]
    assert rs.api.jit_cache_file(S, U, R, G, NT, 8, group=True) == names[0]


def test_the_resident_flag_needs_the_group_flag(rs, tmp_path, monkeypatch):
    monkeypatch.setenv("RS_JIT_CACHE_DIR", str(tmp_path))
    S, U, R, G, NT = SMALL
    L = rs.lib()
    buf = C.create_string_buffer(b"x", 4096)
    assert L.rs_jit_cache_file(S, U, R, G, NT, 8, 1 | 16, buf, 4096) == 0 and buf.value == b""
    err = C.create_string_buffer(4096)
    assert L.rs_jit_cache_warm(S, U, R, G, NT, 8, 1 | 16, err, 4096) < 0 and b"16" in err.value
    assert not list(tmp_path.glob("*.rsco"))
    with pytest.raises(ValueError):
        rs.api.jit_cache_file(S, U, R, G, NT, 8, resident=True)
