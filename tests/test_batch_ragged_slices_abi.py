"""Cells of different slice counts in one batch (not gpu): rs_batch_set_cell_configs_n, rs_batch_cell_slices and
rs_jit_selfcheck_ragged_slices are declared, exported and listed as additions to ABI 11 -- no struct changed its size, the launch
block's pinned gaps hold, "a cell has fewer slices" being a bit of cell_cfg and the count a marker in the device row of eps --; the
binding pads a smaller configuration's rows; and the batch kernel of such a batch compiles, general and lean, at the two shapes the
reference's slice-count sweeps have (20 x 100 users on 64 RBGs of 8 and on 25 RBGs of 4).

What needs a batch handle -- the validation messages, the NULL equivalence, the getters, the checkpoint hash and the grant bound -- needs
a device: tests/test_gpu_batch_ragged_slices.py."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from test_group_run_counted_abi import ROOT, _probe

NEW = ("rs_batch_set_cell_configs_n", "rs_batch_cell_slices", "rs_jit_selfcheck_ragged_slices")
SHAPES = ((20, 100, 64, 8, 512), (20, 100, 25, 4, 512))   # slices, users, RBGs, PRBs per RBG, threads


def test_the_symbols_are_exported_and_listed(rs):
    for name in NEW:
        assert hasattr(rs.lib(), name), f"{name}: declared but not exported"
        assert name in rs.api.ABI_SYMBOLS
    assert rs.api.ABI_SYMBOLS.index("rs_batch_set_cell_configs_n") == rs.api.ABI_SYMBOLS.index("rs_batch_cell_users") + 1
    assert rs.api.ABI_SYMBOLS.index("rs_batch_cell_slices") == rs.api.ABI_SYMBOLS.index("rs_batch_cell_users") + 2
    assert rs.api.ABI_SYMBOLS.index("rs_jit_selfcheck_ragged_slices") == rs.api.ABI_SYMBOLS.index("rs_jit_selfcheck_ragged_cells") + 1
    assert callable(rs.BatchScheduler.cell_slices)
    assert rs.lib().rs_abi_version() == 11 and rs.api.RS_ABI_VERSION == 11


def test_the_header_has_the_prototypes(rs, tmp_path):
    """A C probe against the public header: the entry points have the stated types (-Werror), the version and the three call structs
    are where they were."""
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "radiosaber_hip.h"\n'
                   'typedef int (*set_fn)(rs_batch*, const int32_t*, const double*, const int32_t*, const int32_t*, const int32_t*);\n'
                   'typedef int (*count_fn)(rs_batch*, int32_t*);\n'
                   'typedef int (*check_fn)(int, int, int, int, int, int, int, char*, size_t);\n'
                   'set_fn f0 = rs_batch_set_cell_configs_n;\ncount_fn f1 = rs_batch_cell_slices;\ncheck_fn f2 = rs_jit_selfcheck_ragged_slices;\n'
                   'int main(void) { printf("%d %zu %zu %zu\\n", RS_ABI_VERSION, sizeof(rs_config), sizeof(rs_tti_in), sizeof(rs_tti_out));\n'
                   '  return !f0 || !f1 || !f2; }\n')
    exe = tmp_path / "probe"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), str(rs.build.LIB), f"-Wl,-rpath,{rs.build.LIB.parent}",
                    "-o", str(exe)], check=True)
    abi, cfg, tin, tout = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert abi == 11
    assert (cfg, tin, tout) == (88, 96, 72)
    assert (cfg, tin, tout) == (C.sizeof(rs.api._Config), C.sizeof(rs.api._TtiIn), C.sizeof(rs.api._TtiOut))


def test_a_null_handle_is_invalid(rs):
    L = rs.lib()
    for rc in (L.rs_batch_set_cell_configs_n(None, None, None, None, None, None), L.rs_batch_cell_slices(None, None)):
        assert rc == -1
        assert "null" in L.rs_last_error().decode()


def test_the_launch_block_did_not_move_and_fewer_slices_is_a_bit_of_cell_cfg(tmp_path):
    out = _probe(tmp_path, "ragged_slices_gaps",
                 '  printf("%zu %zu %zu %zu %zu %zu\\n", offsetof(RsLaunch, grp_cbytes) - offsetof(RsLaunch, prio_sum),\n'
                 '    offsetof(RsLaunch, grp_qavg) - offsetof(RsLaunch, grp_cbytes), offsetof(RsLaunch, grp_in) - offsetof(RsLaunch, grp_qavg),\n'
                 '    offsetof(RsLaunch, grp_image) - offsetof(RsLaunch, grp_count), offsetof(RsLaunch, grp_avg) - offsetof(RsLaunch, grp_prb_stride),\n'
                 '    sizeof(RsLaunch) - offsetof(RsLaunch, grp_avg));\n'
                 '  printf("%zu %zu %d %d %d\\n", offsetof(RsLaunch, cell_cfg) - offsetof(RsLaunch, queue_mode), offsetof(RsLaunch, alpha) - offsetof(RsLaunch, queue_mode),\n'
                 '    RS_CELL_CFG_RAGGED, RS_CELL_CFG_SLICES, RS_EPS_ABSENT);')
    # (the bit lies above the two values of the word; the marker is no value algo_epsilon takes in a batch: 0 or 1)
    assert [int(x) for x in out] == [8, 32, 48, 8, 8, 40, 4, 8, 2, 4, -1]


def test_the_binding_takes_configurations_of_fewer_slices(rs):
    """set_cell_configs pads weights with 0 and the exponents with 1 (seen through the arrays it would pass); the maps of smaller
    configurations name their own slices only"""
    cfgs = [rs.SliceConfig([3, 0, 2]), rs.SliceConfig([4, 4]), rs.SliceConfig([8])]
    m = rs.BatchScheduler.padded_maps(cfgs, 8)
    np.testing.assert_array_equal(m, [[0, 0, 0, 2, 2, -1, -1, -1], [0, 0, 0, 0, 1, 1, 1, 1], [0] * 8])
    assert [c.n_slices for c in cfgs] == [3, 2, 1]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(x) for x in s[:4]))
@pytest.mark.parametrize("sched", [7, 8, 9, 10])
def test_both_builds_of_a_batch_with_fewer_slices_compile(rs, sched, shape):
    S, U, R, G, NT = shape
    assert rs.api.jit_selfcheck_cell_configs(S, U, R, G, threads=NT, sched=sched, ragged_slices=True) > 0
    assert rs.api.jit_selfcheck_cell_configs(S, U, R, G, threads=NT, sched=sched, lean=True, ragged_slices=True) > 0


def test_scheduler_11_has_no_such_build(rs):
    S, U, R, G, NT = SHAPES[1]
    buf = C.create_string_buffer(4096)
    assert rs.lib().rs_jit_selfcheck_ragged_slices(S, U, R, G, NT, 11, 0, buf, 4096) < 0
    assert "scheduler 11" in buf.value.decode(errors="replace")
