"""rs_group_specialize_run / rs_group_run_jit_status / rs_jit_selfcheck_group_run (not gpu): declared, exported and listed as additions
to ABI 11 (no struct moved); the null handle is invalid; the general and the lean build of the run kernel compile without a GPU for every
scheduler a run serves, and not for schedulers 7 and 11; flag value 256 of rs_jit_cache_file / rs_jit_cache_warm is valid only together
with 8 and 16, never with 32, 64 or 128, never for schedulers 7 and 11, and every other combination names its reason; the four resident
builds and the two run builds of one shape never share a cache file."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "radiosaber_hip.h"
NEW = ("rs_group_specialize_run", "rs_group_run_jit_status", "rs_jit_selfcheck_group_run")
SMALL = (5, 14, 12, 2, 256)      # slices, users, RBGs, PRBs per RBG, threads: the small shape of tests/test_group_specialize_abi.py
SORT = (20, 100, 64, 8, 512)     # 1 280 sort records on 512 threads: the sort shape of tests/test_group_resident_specialize_abi.py
RUN_SCHEDS = (1, 8, 9, 10, 101, 103)


def test_the_entry_points_are_declared_exported_and_listed(rs, tmp_path):
    txt = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    assert re.search(r"\bint\s+rs_group_specialize_run\s*\(\s*rs_group\s*\*\s*\w+\s*\)", txt)
    assert re.search(r"\bint\s+rs_group_run_jit_status\s*\(\s*rs_group\s*\*\s*\w+\s*,\s*char\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*\)", txt)
    assert re.search(r"\bint\s+rs_jit_selfcheck_group_run\s*\(\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,"
                     r"\s*int\s+\w+\s*,\s*char\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*\)", txt)
    for name in NEW:
        assert hasattr(rs.lib(), name), f"{name} is declared but not exported"
        assert name in rs.api.ABI_SYMBOLS
    for attr in ("specialize_run", "run_jit_status"):
        assert callable(getattr(rs.GroupScheduler, attr))
    # additions: the version and the three call structs are where they were
    assert rs.lib().rs_abi_version() == 11 and rs.api.RS_ABI_VERSION == 11
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "radiosaber_hip.h"\n'
                   'typedef int (*spec_fn)(rs_group*);\ntypedef int (*status_fn)(rs_group*, char*, size_t);\n'
                   'typedef int (*check_fn)(int, int, int, int, int, int, char*, size_t);\n'
                   'enum { declared = sizeof((spec_fn)rs_group_specialize_run) + sizeof((status_fn)rs_group_run_jit_status) + '
                   'sizeof((check_fn)rs_jit_selfcheck_group_run) }; /* (the prototypes are what this line checks) */\n'
                   'int main(void) { printf("%d %zu %zu %zu\\n", RS_ABI_VERSION, sizeof(rs_config), sizeof(rs_tti_in), sizeof(rs_tti_out)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    abi, cfg, tin, tout = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert abi == 11
    assert (cfg, tin, tout) == (88, 96, 72)
    assert (cfg, tin, tout) == (C.sizeof(rs.api._Config), C.sizeof(rs.api._TtiIn), C.sizeof(rs.api._TtiOut))


def test_the_null_handle_is_invalid(rs):
    L = rs.lib()
    assert L.rs_group_specialize_run(None) == -1  # RS_ERR_INVALID
    assert "null" in L.rs_last_error().decode()
    buf = C.create_string_buffer(b"untouched", 64)
    assert L.rs_group_run_jit_status(None, buf, 64) == -1
    assert buf.value == b"untouched"
    assert L.rs_group_run_jit_status(None, None, 0) == -1


@pytest.mark.parametrize("sched", RUN_SCHEDS)
def test_both_run_builds_compile_at_the_small_shape(rs, sched):
    S, U, R, G, NT = SMALL
    assert rs.jit_selfcheck(S, U, R, G, threads=NT, sched=sched, group=True, resident=True, run=True) > 0


def test_both_run_builds_compile_at_the_sort_shape(rs):
    S, U, R, G, NT = SORT
    assert rs.jit_selfcheck(S, U, R, G, threads=NT, sched=9, group=True, resident=True, run=True) > 0


@pytest.mark.parametrize("sched", [7, 11])
def test_schedulers_7_and_11_have_no_run_build(rs, sched):
    S, U, R, G, NT = SMALL
    buf = C.create_string_buffer(4096)
    assert rs.lib().rs_jit_selfcheck_group_run(S, U, R, G, NT, sched, buf, 4096) < 0
    log = buf.value.decode(errors="replace")
    assert f"scheduler {sched}" in log and "run" in log, log
    with pytest.raises(rs.RadioSaberError):
        rs.jit_selfcheck(S, U, R, G, threads=NT, sched=sched, group=True, resident=True, run=True)


def test_the_fault_injection_hook_is_a_build_of_its_own_and_compiles(rs, tmp_path, monkeypatch):
    """RS_FAULT_INJECT_RUN (tests only; no shipped build defines it) compiles in both builds, and its option list is a key of its own."""
    monkeypatch.setenv("RS_JIT_CACHE_DIR", str(tmp_path))
    S, U, R, G, NT = SMALL
    plain = rs.api.jit_cache_file(S, U, R, G, NT, 9, group=True, resident=True, run=True)
    monkeypatch.setenv("RS_JIT_EXTRA", "-DRS_FAULT_INJECT_RUN")
    assert rs.api.jit_cache_file(S, U, R, G, NT, 9, group=True, resident=True, run=True) != plain
    assert rs.jit_selfcheck(S, U, R, G, threads=NT, sched=9, group=True, resident=True, run=True) > 0


@pytest.mark.parametrize("flags,sched,reason", [
    (1 | 256, 9, "only together with 8"),                      # no group flag
    (1 | 8 | 256, 9, "and 16"),                                # a group's build, but not the resident form
    (1 | 4 | 8 | 256, 9, "and 16"),
    (1 | 16 | 256, 9, "only together with 8"),                 # the resident flag without the group flag
    (1 | 8 | 32 | 256, 9, "and 16"),                           # the queued form instead of the resident one
    (1 | 8 | 16 | 32 | 256, 9, "excludes 32"),
    (1 | 8 | 16 | 64 | 256, 9, "64"),
    (1 | 8 | 16 | 32 | 64 | 256, 9, "64"),
    (1 | 8 | 16 | 128 | 256, 1, "128"),
    (1 | 8 | 128 | 256, 1, "and 16"),
    (1 | 8 | 16 | 256, 7, "schedulers 7 and 11"),
    (1 | 4 | 8 | 16 | 256, 11, "schedulers 7 and 11"),
])
def test_every_invalid_combination_of_flag_256_names_its_reason(rs, tmp_path, monkeypatch, flags, sched, reason):
    monkeypatch.setenv("RS_JIT_CACHE_DIR", str(tmp_path))
    S, U, R, G, NT = SMALL
    L = rs.lib()
    buf = C.create_string_buffer(b"x", 4096)
    assert L.rs_jit_cache_file(S, U, R, G, NT, sched, flags, buf, 4096) == 0 and buf.value == b""
    err = C.create_string_buffer(4096)
    assert L.rs_jit_cache_warm(S, U, R, G, NT, sched, flags, err, 4096) < 0
    msg = err.value.decode()
    assert "256" in msg and "the run form" in msg and reason in msg, msg
    assert not list(tmp_path.glob("*.rsco"))


def test_the_python_flags_refuse_what_the_library_refuses(rs):
    S, U, R, G, NT = SMALL
    for kw in (dict(run=True), dict(group=True, run=True), dict(resident=True, run=True),
               dict(group=True, resident=True, run=True, flows=True), dict(group=True, queued=True, run=True)):
        with pytest.raises(ValueError):
            rs.api.jit_cache_file(S, U, R, G, NT, 9, **kw)


def test_the_resident_and_the_run_builds_have_six_cache_files(rs, tmp_path, monkeypatch):
    monkeypatch.setenv("RS_JIT_CACHE_DIR", str(tmp_path))
    monkeypatch.delenv("RS_JIT_CACHE", raising=False)
    monkeypatch.delenv("RS_JIT_EXTRA", raising=False)
    S, U, R, G, NT = SMALL
    L = rs.lib()
    all_flags = (1 | 8, 1 | 4 | 8, 1 | 8 | 16, 1 | 4 | 8 | 16, 1 | 8 | 16 | 256, 1 | 4 | 8 | 16 | 256)
    names = []
    for flags in all_flags:   # the plain, the resident and the run kernel of a group, general and lean
        buf = C.create_string_buffer(4096)
        assert L.rs_jit_cache_file(S, U, R, G, NT, 8, flags, buf, 4096) > 0
        names.append(buf.value.decode())
    assert len(set(names)) == 6, names
    before = rs.jit_cache_stats()
    err = C.create_string_buffer(4096)
    assert L.rs_jit_cache_warm(S, U, R, G, NT, 8, 1 | 8 | 16, err, 4096) > 0, err.value
    assert L.rs_jit_cache_warm(S, U, R, G, NT, 8, 1 | 8 | 16 | 256, err, 4096) > 0, err.value
    assert L.rs_jit_cache_warm(S, U, R, G, NT, 8, 1 | 4 | 8 | 16 | 256, err, 4096) > 0, err.value
    files = sorted(str(f) for f in tmp_path.glob("*.rsco"))
    assert files == sorted([names[2], names[4], names[5]]), (files, names)
    after = rs.jit_cache_stats()
    assert after["misses"] - before["misses"] == 3 and after["stores"] - before["stores"] == 3
    # the key text in the file says which is which
    texts = {f: Path(f).read_bytes() for f in files}
    assert b"-DRS_JIT_GROUP_RUN=1" not in texts[names[2]]
    for n in (4, 5):
        assert b"-DRS_JIT_GROUP_RUN=1" in texts[names[n]] and b"-DRS_JIT_GROUP_RESIDENT=1" in texts[names[n]] and b"-DRS_JIT_GROUP=1" in texts[names[n]]
    assert b"-DRS_JIT_LEAN=1" in texts[names[5]] and b"-DRS_JIT_LEAN=1" not in texts[names[4]]
    # and each is found again under its own key
    for n, flags in enumerate((1 | 8 | 16, 1 | 8 | 16 | 256, 1 | 4 | 8 | 16 | 256)):
        assert L.rs_jit_cache_warm(S, U, R, G, NT, 8, flags, err, 4096) > 0
        assert rs.jit_cache_stats()["hits"] - after["hits"] == n + 1
    assert sorted(str(f) for f in tmp_path.glob("*.rsco")) == files
    assert rs.api.jit_cache_file(S, U, R, G, NT, 8, group=True, resident=True, run=True) == names[4]
    assert rs.api.jit_cache_file(S, U, R, G, NT, 8, group=True, resident=True, run=True, lean=True) == names[5]
    assert rs.api.jit_cache_file(S, U, R, G, NT, 8, group=True, resident=True) == names[2]
