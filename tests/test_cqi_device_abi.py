"""CQI epoch grids from device memory (not gpu): rs_batch_set_cqi_epochs_device, rs_batch_write_cqi_epochs_device,
rs_batch_cqi_write_status and rs_batch_debug_cqi_image are declared with the stated types, exported, listed directly behind
rs_batch_download_cqi_epochs and callable from the binding -- additions to ABI 11, no struct changed its size."""
import ctypes as C
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
NEW = ("rs_batch_set_cqi_epochs_device", "rs_batch_write_cqi_epochs_device", "rs_batch_cqi_write_status", "rs_batch_debug_cqi_image")


def test_the_symbols_are_exported_and_listed_behind_the_download(rs):
    at = rs.api.ABI_SYMBOLS.index("rs_batch_download_cqi_epochs")
    assert tuple(rs.api.ABI_SYMBOLS[at + 1:at + 5]) == NEW
    for name in NEW:
        assert hasattr(rs.lib(), name), f"{name}: declared but not exported"
        assert getattr(rs.lib(), name).argtypes == rs.api.PROTOTYPES[name][1]
    for method in ("set_cqi_epochs_device", "write_cqi_epochs_device", "cqi_write_status", "debug_cqi_image"):
        assert callable(getattr(rs.BatchScheduler, method))
    assert rs.api.RS_CQI_WRITE_ASYNC == 1
    assert rs.lib().rs_abi_version() == 11 and rs.api.RS_ABI_VERSION == 11


def test_the_header_has_the_prototypes_and_the_flag(rs, tmp_path):
    """A C99 probe against the public header under -Wall -Werror: the four entry points have the stated types, RS_CQI_WRITE_ASYNC is
    the unsigned 1, the version and the three call structs are where they were."""
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "radiosaber_hip.h"\n'
                   'typedef int (*set_fn)(rs_batch*, const uint8_t*, size_t, int32_t);\n'
                   'typedef int (*write_fn)(rs_batch*, int32_t, int32_t, const uint8_t*, size_t, uint32_t);\n'
                   'typedef int (*status_fn)(rs_batch*, int64_t*, int32_t*);\n'
                   'typedef int (*image_fn)(rs_batch*, int32_t, int32_t, uint8_t*, size_t);\n'
                   'set_fn f0 = rs_batch_set_cqi_epochs_device;\nwrite_fn f1 = rs_batch_write_cqi_epochs_device;\n'
                   'status_fn f2 = rs_batch_cqi_write_status;\nimage_fn f3 = rs_batch_debug_cqi_image;\n'
                   'int main(void) { printf("%u %d %d %zu %zu %zu\\n", RS_CQI_WRITE_ASYNC, (RS_CQI_WRITE_ASYNC - 2) > 0, RS_ABI_VERSION,\n'
                   '    sizeof(rs_config), sizeof(rs_tti_in), sizeof(rs_tti_out));\n'
                   '  return !f0 || !f1 || !f2 || !f3; }\n')
    exe = tmp_path / "probe"
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), str(rs.build.LIB), f"-Wl,-rpath,{rs.build.LIB.parent}",
                    "-o", str(exe)], check=True)
    flag, unsigned, abi, cfg, tin, tout = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert flag == 1 and unsigned == 1 and abi == 11
    assert (cfg, tin, tout) == (88, 96, 72)
    assert (cfg, tin, tout) == (C.sizeof(rs.api._Config), C.sizeof(rs.api._TtiIn), C.sizeof(rs.api._TtiOut))


def test_a_null_handle_is_invalid_for_all_four(rs):
    L = rs.lib()
    buf = (C.c_uint8 * 16)()
    byte, value = C.c_int64(7), C.c_int32(7)
    assert L.rs_batch_set_cqi_epochs_device(None, C.addressof(buf), 16, 1) == -1
    assert L.rs_batch_write_cqi_epochs_device(None, 0, 1, C.addressof(buf), 16, 0) == -1
    assert L.rs_batch_cqi_write_status(None, C.byref(byte), C.byref(value)) == -1
    assert "null" in L.rs_last_error().decode()
    assert L.rs_batch_debug_cqi_image(None, 0, 0, buf, 16) == -1
    assert (byte.value, value.value) == (7, 7)  # a refusal stores nothing


def test_the_binding_checks_the_tensor_before_any_call(rs):
    """ValueError from the Python checks alone: no batch exists here (no GPU), so a call into the library would fail otherwise"""
    import pytest

    class Fake:
        n_cells, U, R, device = 3, 7, 25, 0
    for bad in (object(), [[1]]):
        with pytest.raises(ValueError, match="torch tensor"):
            rs.BatchScheduler._device_grids(Fake(), bad, "set_cqi_epochs_device")

    class CpuTensor:  # what the checks read of a torch tensor, and nothing else
        is_cuda, dtype, shape = False, "torch.uint8", (3, 5, 7, 25)
        device = type("Device", (), {"index": None, "__str__": lambda self: "cpu"})()
        data_ptr = is_contiguous = element_size = staticmethod(lambda: 1)
    with pytest.raises(ValueError, match="not on the batch's device"):
        rs.BatchScheduler._device_grids(Fake(), CpuTensor(), "set_cqi_epochs_device")
