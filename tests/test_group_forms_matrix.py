"""The forms of a group call x the schedulers (not gpu): which run-time builds exist.  One matrix -- rs_group_form_serves of
csrc/rs_device.h, the kernels the library carries -- answers for rs_jit_cache_file and for the rs_jit_selfcheck_group_* exports that
refuse schedulers; the one cell where the cache functions answer differently (plain and resident builds are never asked for their
scheduler, so 11 passes there) is pinned as it is.  Only refusals are called: they return before any compile."""
import ctypes as C

import pytest

SCHEDS = (1, 7, 8, 9, 10, 11, 101, 103)
SHAPE = (4, 40, 13, 4, 512)  # slices, users, RBGs, PRBs per RBG, threads
#          scheduler:     1  7  8  9 10 11 101 103
MATRIX = {"plain":    "y y y y y - y y".split(),
          "resident": "y y y y y - y y".split(),
          "queued":   "- y y y - - y y".split(),
          "counted":  "- y y y - - y y".split(),
          "flows":    "y - - - - - - -".split(),
          "run":      "y - y y y - y y".split()}
FLAGS = {"plain": 8, "resident": 8 | 16, "queued": 8 | 32, "counted": 8 | 32 | 64, "flows": 8 | 128, "run": 8 | 16 | 256}
REFUSAL = {"queued": "scheduler %d has no queued form (rs_group_queued_kernel exists for 7, 8, 9, 101 and 103)",
           "counted": "scheduler %d has no counted form (rs_group_counted_kernel exists for 7, 8, 9, 101 and 103)",
           "flows": "scheduler %d has no flows form (rs_group_flows_kernel exists for scheduler 1)",
           "run": "scheduler %d has no run form (rs_group_run_kernel exists for 1, 8, 9, 10, 101 and 103)"}


def served(form, sched):
    return MATRIX[form][SCHEDS.index(sched)] == "y"


@pytest.mark.parametrize("form", list(MATRIX))
def test_a_cache_file_exists_exactly_for_the_served_cells(rs, form, monkeypatch, tmp_path):
    monkeypatch.setenv("RS_JIT_CACHE_DIR", str(tmp_path))
    L = rs.lib()
    for sched in SCHEDS:
        for lean in (0, 4):
            buf = C.create_string_buffer(512)
            n = L.rs_jit_cache_file(*SHAPE, sched, FLAGS[form] | lean, buf, 512)
            # the exception: plain and resident builds of scheduler 11, which no group kernel serves
            want = served(form, sched) or (sched == 11 and form in ("plain", "resident"))
            assert (n > 0) == want and (buf.value != b"") == want, (form, sched, lean, buf.value)


@pytest.mark.parametrize("form", list(REFUSAL))
def test_the_self_checks_refuse_exactly_the_unserved_cells(rs, form):
    fn = getattr(rs.lib(), "rs_jit_selfcheck_group_" + form)
    for sched in SCHEDS:
        if served(form, sched):
            continue  # (a served cell compiles: the tests/test_group_*_specialize_abi.py files do that)
        err = C.create_string_buffer(512)
        assert fn(*SHAPE, sched, err, 512) == -1
        assert err.value.decode() == REFUSAL[form] % sched
