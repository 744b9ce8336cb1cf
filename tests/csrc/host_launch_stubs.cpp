// Sanitizer build only (tools/sanitize_cpu.sh): the HOST side of the library -- rs_api.cpp + rs_jit.cpp compiled by g++ with
// -fsanitize=address,undefined -- has no device code, so the kernel launchers of rs_kernels.hip resolve to these refusals.
// Nothing here computes anything: without a GPU every entry point that would launch has already returned RS_ERR_NO_DEVICE.
// The launchers' one declaration is rs_host.h: a stub that disagrees with it does not compile, one that is missing does not link
// (tests/test_jit_option_lists.py links the three files with --no-undefined).
#include "../../radiosaber_amd/csrc/rs_host.h"
extern "C" hipError_t rs_launch_cells(const RsLaunch*, int, hipStream_t) { return hipErrorNotSupported; }
extern "C" hipError_t rs_launch_group(const RsLaunch*, int, int, hipStream_t) { return hipErrorNotSupported; }
extern "C" hipError_t rs_prepare_kernels(int) { return hipErrorNotSupported; }
extern "C" hipError_t rs_launch_synth(uint8_t*, int64_t, int, int, int, int, int, uint64_t, int64_t, const uint32_t*, hipStream_t) { return hipErrorNotSupported; }
extern "C" hipError_t rs_launch_pack_cqi(const uint8_t*, uint8_t*, unsigned long long*, int, int, int, int, int, int, int, int64_t, hipStream_t) { return hipErrorNotSupported; }
extern "C" hipError_t rs_launch_copy_probe(const void*, void*, size_t, hipStream_t) { return hipErrorNotSupported; }
extern "C" hipError_t rs_launch_slice_totals(const int64_t*, const int64_t*, const uint8_t*, int64_t, int, int, int, long long*, hipStream_t) { return hipErrorNotSupported; }
extern "C" hipError_t rs_launch_slice_bytes(const int64_t*, const uint8_t*, int64_t, int, int, int, unsigned long long*, hipStream_t) { return hipErrorNotSupported; }
