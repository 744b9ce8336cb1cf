"""Per-cell configurations of a batch (not gpu): rs_batch_set_cell_configs, rs_batch_get_cell_config, rs_batch_slice_totals and
rs_jit_selfcheck_cell_configs are declared, exported and listed; they are additions to ABI 11 -- the call structs keep their sizes, the
launch block took its one new word out of the padding behind queue_mode and its pinned gaps hold --, and the batch kernel with per-cell
rows compiles, general and lean, for every scheduler that has it."""
import ctypes as C
import subprocess

import pytest

from test_group_run_counted_abi import ROOT, _probe

NEW = ("rs_batch_set_cell_configs", "rs_batch_get_cell_config", "rs_batch_slice_totals", "rs_jit_selfcheck_cell_configs")
SHAPE = (4, 96, 6, 2, 512)    # slices, users, RBGs, PRBs per RBG, threads: the shape of tests/test_gpu_batch_cell_configs.py


def test_the_symbols_are_exported_and_listed(rs):
    for name in NEW:
        assert hasattr(rs.lib(), name), f"{name}: declared but not exported"
        assert name in rs.api.ABI_SYMBOLS
    order = [rs.api.ABI_SYMBOLS.index(n) for n in NEW]
    assert order[:3] == [rs.api.ABI_SYMBOLS.index("rs_batch_seed") + k for k in (1, 2, 3)]     # next to rs_batch_seed, as in the header
    assert order[3] == rs.api.ABI_SYMBOLS.index("rs_jit_selfcheck_grant_records") + 1
    for attr in ("set_cell_configs", "cell_config", "slice_totals"):
        assert callable(getattr(rs.BatchScheduler, attr))
    assert rs.lib().rs_abi_version() == 11 and rs.api.RS_ABI_VERSION == 11


def test_the_prototypes_and_the_struct_sizes(rs, tmp_path):
    """A C probe against the public header: each entry point is assigned to a pointer of its type (an incompatible one stops the build
    under -Werror); the version and the three call structs are where they were."""
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "radiosaber_hip.h"\n'
                   'typedef int (*set_fn)(rs_batch*, const double*, const int32_t*, const int32_t*, const int32_t*);\n'
                   'typedef int (*get_fn)(rs_batch*, int32_t, double*, int32_t*, int32_t*, int32_t*);\n'
                   'typedef int (*totals_fn)(rs_batch*, int64_t*, int64_t*);\n'
                   'typedef int (*check_fn)(int, int, int, int, int, int, int, char*, size_t);\n'
                   'set_fn f0 = rs_batch_set_cell_configs;\nget_fn f1 = rs_batch_get_cell_config;\n'
                   'totals_fn f2 = rs_batch_slice_totals;\ncheck_fn f3 = rs_jit_selfcheck_cell_configs;\n'
                   'int main(void) { printf("%d %zu %zu %zu\\n", RS_ABI_VERSION, sizeof(rs_config), sizeof(rs_tti_in), sizeof(rs_tti_out));\n'
                   '  return !f0 || !f1 || !f2 || !f3; }\n')
    exe = tmp_path / "probe"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), str(rs.build.LIB), f"-Wl,-rpath,{rs.build.LIB.parent}",
                    "-o", str(exe)], check=True)
    abi, cfg, tin, tout = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert abi == 11
    assert (cfg, tin, tout) == (88, 96, 72)
    assert (cfg, tin, tout) == (C.sizeof(rs.api._Config), C.sizeof(rs.api._TtiIn), C.sizeof(rs.api._TtiOut))


def test_a_null_handle_is_invalid(rs):
    L = rs.lib()
    for rc in (L.rs_batch_set_cell_configs(None, None, None, None, None), L.rs_batch_get_cell_config(None, 0, None, None, None, None),
               L.rs_batch_slice_totals(None, None, None)):
        assert rc == -1
        assert "null" in L.rs_last_error().decode()


def test_the_launch_block_did_not_move(tmp_path):
    """The pinned gaps of RsLaunch (tests/test_batch_records_abi.py) as they were, and the new word where the issue puts it: in the four
    bytes of padding between queue_mode and the pointer behind it."""
    out = _probe(tmp_path, "gaps",
                 '  printf("%zu %zu %zu %zu %zu %zu\\n", offsetof(RsLaunch, grp_cbytes) - offsetof(RsLaunch, prio_sum),\n'
                 '    offsetof(RsLaunch, grp_qavg) - offsetof(RsLaunch, grp_cbytes), offsetof(RsLaunch, grp_in) - offsetof(RsLaunch, grp_qavg),\n'
                 '    offsetof(RsLaunch, grp_image) - offsetof(RsLaunch, grp_count), offsetof(RsLaunch, grp_avg) - offsetof(RsLaunch, grp_prb_stride),\n'
                 '    sizeof(RsLaunch) - offsetof(RsLaunch, grp_avg));\n'
                 '  printf("%zu %zu %d\\n", offsetof(RsLaunch, cell_cfg) - offsetof(RsLaunch, queue_mode), offsetof(RsLaunch, alpha) - offsetof(RsLaunch, queue_mode),\n'
                 '    offsetof(RsLaunch, cell_cfg) < offsetof(RsLaunch, prio_sum));')
    assert [int(x) for x in out] == [8, 32, 48, 8, 8, 40, 4, 8, 1]


@pytest.mark.parametrize("sched", [1, 7, 8, 9, 10, 101, 103])
def test_both_builds_with_per_cell_rows_compile(rs, sched):
    S, U, R, G, NT = SHAPE
    assert rs.api.jit_selfcheck_cell_configs(S, U, R, G, threads=NT, sched=sched) > 0
    assert rs.api.jit_selfcheck_cell_configs(S, U, R, G, threads=NT, sched=sched, lean=True) > 0


def test_scheduler_11_has_no_build_with_per_cell_rows(rs):
    S, U, R, G, NT = SHAPE
    buf = C.create_string_buffer(4096)
    assert rs.lib().rs_jit_selfcheck_cell_configs(S, U, R, G, NT, 11, 0, buf, 4096) < 0
    assert "scheduler 11" in buf.value.decode(errors="replace")
    with pytest.raises(rs.RadioSaberError):
        rs.api.jit_selfcheck_cell_configs(S, U, R, G, threads=NT, sched=11, lean=True)
