"""Cells of different user counts in one batch (not gpu): RS_USER_ABSENT, rs_batch_cell_users and rs_jit_selfcheck_ragged_cells are
declared, exported and listed as additions to ABI 11 -- no struct changed its size and the launch block's pinned gaps hold, the word
that says "ragged" being a value of cell_cfg --; the binding pads a smaller configuration's map with RS_USER_ABSENT; and the batch
kernel of a ragged batch compiles, general and lean, for every scheduler that has per-cell rows."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from test_group_run_counted_abi import ROOT, _probe

NEW = ("rs_batch_cell_users", "rs_jit_selfcheck_ragged_cells")
SHAPE = (4, 96, 6, 2, 512)    # slices, users, RBGs, PRBs per RBG, threads: the shape of tests/test_gpu_batch_ragged_cells.py


def test_the_symbols_are_exported_and_listed(rs):
    for name in NEW:
        assert hasattr(rs.lib(), name), f"{name}: declared but not exported"
        assert name in rs.api.ABI_SYMBOLS
    assert rs.api.ABI_SYMBOLS.index("rs_batch_cell_users") == rs.api.ABI_SYMBOLS.index("rs_batch_slice_totals") + 1
    assert rs.api.ABI_SYMBOLS.index("rs_jit_selfcheck_ragged_cells") == rs.api.ABI_SYMBOLS.index("rs_jit_selfcheck_cell_configs") + 1
    assert callable(rs.BatchScheduler.cell_users)
    assert rs.api.RS_USER_ABSENT == -1
    assert rs.lib().rs_abi_version() == 11 and rs.api.RS_ABI_VERSION == 11


def test_the_header_has_the_value_and_the_prototypes(rs, tmp_path):
    """A C probe against the public header: RS_USER_ABSENT is -1, the entry points have the stated types (-Werror), the version and
    the three call structs are where they were."""
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "radiosaber_hip.h"\n'
                   'typedef int (*users_fn)(rs_batch*, int32_t*);\n'
                   'typedef int (*check_fn)(int, int, int, int, int, int, int, char*, size_t);\n'
                   'users_fn f0 = rs_batch_cell_users;\ncheck_fn f1 = rs_jit_selfcheck_ragged_cells;\n'
                   'int main(void) { printf("%d %d %zu %zu %zu\\n", RS_USER_ABSENT, RS_ABI_VERSION, sizeof(rs_config), sizeof(rs_tti_in), sizeof(rs_tti_out));\n'
                   '  return !f0 || !f1; }\n')
    exe = tmp_path / "probe"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), str(rs.build.LIB), f"-Wl,-rpath,{rs.build.LIB.parent}",
                    "-o", str(exe)], check=True)
    absent, abi, cfg, tin, tout = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert absent == -1 and abi == 11
    assert (cfg, tin, tout) == (88, 96, 72)
    assert (cfg, tin, tout) == (C.sizeof(rs.api._Config), C.sizeof(rs.api._TtiIn), C.sizeof(rs.api._TtiOut))


def test_a_null_handle_is_invalid(rs):
    L = rs.lib()
    assert L.rs_batch_cell_users(None, None) == -1
    assert "null" in L.rs_last_error().decode()


def test_the_launch_block_did_not_move_and_ragged_is_a_value_of_cell_cfg(tmp_path):
    out = _probe(tmp_path, "ragged_gaps",
                 '  printf("%zu %zu %zu %zu %zu %zu\\n", offsetof(RsLaunch, grp_cbytes) - offsetof(RsLaunch, prio_sum),\n'
                 '    offsetof(RsLaunch, grp_qavg) - offsetof(RsLaunch, grp_cbytes), offsetof(RsLaunch, grp_in) - offsetof(RsLaunch, grp_qavg),\n'
                 '    offsetof(RsLaunch, grp_image) - offsetof(RsLaunch, grp_count), offsetof(RsLaunch, grp_avg) - offsetof(RsLaunch, grp_prb_stride),\n'
                 '    sizeof(RsLaunch) - offsetof(RsLaunch, grp_avg));\n'
                 '  printf("%zu %zu %d %d\\n", offsetof(RsLaunch, cell_cfg) - offsetof(RsLaunch, queue_mode), offsetof(RsLaunch, alpha) - offsetof(RsLaunch, queue_mode),\n'
                 '    RS_CELL_CFG_RAGGED, RS_SLICE_ABSENT);')
    # (the absent user's byte of the device map lies above every slice id: RS_MAX_SLICES is 64)
    assert [int(x) for x in out] == [8, 32, 48, 8, 8, 40, 4, 8, 2, 255]


def test_the_binding_pads_a_smaller_configurations_map(rs):
    cfgs = [rs.SliceConfig([3, 0, 2]), rs.SliceConfig([1, 1, 1]), rs.SliceConfig([2, 2, 4])]
    m = rs.BatchScheduler.padded_maps(cfgs, 8)
    assert m.dtype == np.int32
    np.testing.assert_array_equal(m, [[0, 0, 0, 2, 2, -1, -1, -1], [0, 1, 2, -1, -1, -1, -1, -1], [0, 0, 1, 1, 2, 2, 2, 2]])


@pytest.mark.parametrize("sched", [1, 7, 8, 9, 10, 101, 103])
def test_both_builds_of_a_ragged_batch_compile(rs, sched):
    S, U, R, G, NT = SHAPE
    assert rs.api.jit_selfcheck_cell_configs(S, U, R, G, threads=NT, sched=sched, ragged=True) > 0
    assert rs.api.jit_selfcheck_cell_configs(S, U, R, G, threads=NT, sched=sched, lean=True, ragged=True) > 0


def test_scheduler_11_has_no_ragged_build(rs):
    S, U, R, G, NT = SHAPE
    buf = C.create_string_buffer(4096)
    assert rs.lib().rs_jit_selfcheck_ragged_cells(S, U, R, G, NT, 11, 0, buf, 4096) < 0
    assert "scheduler 11" in buf.value.decode(errors="replace")
