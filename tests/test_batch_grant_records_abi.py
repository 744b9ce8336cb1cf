"""Grant records of backlogged batches (not gpu): rs_batch_grant_record, rs_batch_grant_bound, rs_batch_run_grant_records and
rs_jit_selfcheck_grant_records are declared, exported and listed; they are additions to ABI 11 -- the record is 32 bytes in the header, in
the numpy dtype and on the device, RsLaunch and the LDS carve did not grow --, and the records variant of the batch kernel compiles in
its general and its lean build for every scheduler that has one."""
import subprocess

import numpy as np
import pytest

from test_group_run_counted_abi import ROOT, _probe

NEW = ("rs_batch_grant_bound", "rs_batch_run_grant_records", "rs_jit_selfcheck_grant_records")
FIELDS = ("tti", "user", "tbs_bits", "bytes", "rbg_mask", "nprb", "final_cqi", "mcs", "reserved")
OFFSETS = [0, 4, 8, 12, 16, 24, 28, 29, 30]
SHAPE = (20, 100, 25, 4, 512)


def test_the_symbols_are_exported_and_listed(rs):
    for name in NEW:
        assert hasattr(rs.lib(), name), f"{name}: declared but not exported"
        assert name in rs.api.ABI_SYMBOLS
    assert callable(rs.BatchScheduler.grant_bound) and callable(rs.BatchScheduler.run_grant_records)
    assert rs.lib().rs_abi_version() == 11


def test_a_null_handle_is_invalid(rs):
    L = rs.lib()
    n = np.zeros(1, np.int64)
    recs = np.zeros(4, rs.api.BATCH_GRANT_RECORD)
    for rc in (L.rs_batch_grant_bound(None),
               L.rs_batch_run_grant_records(None, 1, 4, recs.ctypes.data, n.ctypes.data_as(L.rs_batch_run_grant_records.argtypes[4]))):
        assert rc == -1
        assert "null" in L.rs_last_error().decode()


def test_the_record_is_32_bytes(rs, tmp_path):
    """A C++ probe against the public header: the prototypes (an incompatible pointer type stops the build), the record's size and
    field offsets, the version; the numpy dtype of the Python surface and the device's twin are the same record."""
    src = tmp_path / "probe.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "radiosaber_hip.h"\n'
                   'typedef int (*bound_fn)(rs_batch*);\n'
                   'typedef int (*run_fn)(rs_batch*, int32_t, int64_t, rs_batch_grant_record*, int64_t*);\n'
                   'typedef int (*check_fn)(int, int, int, int, int, int, int, char*, size_t);\n'
                   'bound_fn f0 = rs_batch_grant_bound;\nrun_fn f1 = rs_batch_run_grant_records;\ncheck_fn f2 = rs_jit_selfcheck_grant_records;\n'
                   'int main() { printf("%d %zu", RS_ABI_VERSION, sizeof(rs_batch_grant_record));\n'
                   + "".join(f'  printf(" %zu", offsetof(rs_batch_grant_record, {f}));\n' for f in FIELDS) +
                   '  return !f0 || !f1 || !f2; }\n')
    exe = tmp_path / "probe"
    subprocess.run(["c++", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), str(rs.build.LIB), f"-Wl,-rpath,{rs.build.LIB.parent}",
                    "-o", str(exe)], check=True)
    abi, size, *offs = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert abi == 11
    assert size == 32 and offs == OFFSETS and offs[4] == 16 and offs[5] == 24
    dt = rs.api.BATCH_GRANT_RECORD
    assert dt.itemsize == 32 and [dt.fields[n][1] for n in FIELDS] == offs
    dev = _probe(tmp_path, "dev", '  printf("%zu", sizeof(RsBatchGrantRecord));\n'
                 + "".join(f'  printf(" %zu", offsetof(RsBatchGrantRecord, {f}));\n' for f in FIELDS))
    assert [int(x) for x in dev] == [32] + offs


def test_the_launch_block_and_the_carve_did_not_grow(rs, tmp_path):
    """The record block rides in the pointer pair the bearer records use (no non-queue batch launch set it), scheduler 10's place counter
    came out of RsMisc's padding: RsLaunch's pinned gaps and the LDS carve are what they were."""
    out = _probe(tmp_path, "gaps",
                 '  printf("%zu %zu %zu %zu\\n", offsetof(RsLaunch, grp_cbytes) - offsetof(RsLaunch, prio_sum),\n'
                 '    offsetof(RsLaunch, grp_qavg) - offsetof(RsLaunch, grp_cbytes), sizeof(RsLaunch) - offsetof(RsLaunch, grp_avg),\n'
                 '    sizeof(RsMisc) - offsetof(RsMisc, prio_boost));')
    assert [int(x) for x in out] == [8, 32, 40, 16]
    assert rs.lds_bytes_per_cell(20, 500, 25, rs.RS_SCHED_MAXCELL, 512) == 40960


@pytest.mark.parametrize("lean", [False, True])
@pytest.mark.parametrize("sched", [1, 7, 8, 9, 10, 101, 103])
def test_the_records_variant_compiles(rs, sched, lean):
    assert rs.api.jit_selfcheck_grant_records(*SHAPE, sched, lean=lean) > 0


@pytest.mark.parametrize("lean", [False, True])
@pytest.mark.parametrize("shape", [(20, 100, 64, 8, 512, 9), (3, 12, 25, 4, 64, 9)])
def test_the_records_variant_compiles_on_the_scan_path_and_on_one_wave(rs, shape, lean):
    """above 32 RBGs the lane sets are 64-bit masks (the scan path); with 64 threads wave 0 is the only wave"""
    assert rs.api.jit_selfcheck_grant_records(*shape, lean=lean) > 0


def test_scheduler_11_has_no_records_variant(rs):
    import ctypes as C
    buf = C.create_string_buffer(512)
    assert rs.lib().rs_jit_selfcheck_grant_records(*SHAPE, 11, 0, buf, 512) < 0
    assert "scheduler 11" in buf.value.decode()
    with pytest.raises(rs.RadioSaberError, match="scheduler 11"):
        rs.api.jit_selfcheck_grant_records(*SHAPE, 11)


def test_a_build_without_records_says_so_in_its_options():
    """-DRS_JIT_RECORDS is part of every option list: the records variant has a cache file of its own (and with it a self-check mark of
    its own), told from the plain build's by the option alone."""
    src = (ROOT / "radiosaber_amd" / "csrc" / "rs_jit.cpp").read_text()
    assert 'o.push_back("-DRS_JIT_RECORDS=0")' in src
    api_src = (ROOT / "radiosaber_amd" / "csrc" / "rs_api.cpp").read_text()
    assert '"-DRS_JIT_RECORDS=1"' in api_src
