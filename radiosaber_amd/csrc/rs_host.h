/*
 * rs_host.h -- the internal seam between the library's three translation units, host only (never embedded for hiprtc):
 * the launchers of rs_kernels.hip's host part, the run-time builds of rs_jit.cpp, and their caller rs_api.cpp.  Every symbol that
 * crosses is declared here once and every file that defines or calls one includes this header (tests/csrc/host_launch_stubs.cpp too),
 * so a definition that disagrees is a compile error: with extern "C" it would still link.
 */
#ifndef RS_HOST_H_
#define RS_HOST_H_

#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "rs_device.h"

/* ---- the kernel launchers (rs_kernels.hip) ---- */
extern "C" hipError_t rs_launch_cells(const RsLaunch* p, int threads, hipStream_t stream);
extern "C" hipError_t rs_launch_group(const RsLaunch* p, int threads, int form, hipStream_t stream); /* form: RsGroupFormId */
extern "C" hipError_t rs_prepare_kernels(int max_lds_bytes);
extern "C" hipError_t rs_launch_synth(uint8_t* epochs, int64_t grid_stride, int n_cells, int n_epochs, int U, int R, int Upad,
                                      uint64_t seed, int64_t first_cell, const uint32_t* cdf16, hipStream_t stream);
extern "C" hipError_t rs_launch_pack_cqi(const uint8_t* src, uint8_t* epochs, unsigned long long* bad_word, int n_cells, int n_src,
                                         int first_epoch, int n_epochs, int U, int R, int Upad, int64_t grid_stride,
                                         hipStream_t stream);
extern "C" hipError_t rs_launch_copy_probe(const void* src, void* dst, size_t bytes, hipStream_t stream);
extern "C" hipError_t rs_launch_slice_totals(const int64_t* cum_bytes, const int64_t* cum_rbs, const uint8_t* user_slice, int64_t map_stride,
                                             int n_cells, int U, int S, long long* out, hipStream_t stream);
extern "C" hipError_t rs_launch_slice_bytes(const int64_t* cum_bytes, const uint8_t* user_slice, int64_t map_stride, int n_cells, int U,
                                            int S, unsigned long long* d_out, hipStream_t stream);

/* ---- the run-time builds (rs_jit.cpp) ----
 * What a caller asks a build for.  The option list that follows from it is the disk cache's key and decides which kernel runs.
 *   qmode    rs_carve's `queue` argument: 0 no queue model, 2 queue model with the bearers' hot words in LDS when they fit, 3 queue
 *            model with them in HBM, 1 the gate scratch of a drop-in PF / NVS context
 *   win      the batch's longest 8-aligned slice window (0: unknown; drop-in contexts and group builds)
 *   flags    1 the drop-in entry point's one-TTI form, 2 a batch whose CQI grid changes every few TTIs (cqi_refresh <= 4, the
 *            streamed-CQI mode), 4 the lean build; the rest name a form of a group call (RsGroupForm::jit_flags): 8 a group's build,
 *            16 its resident form, 32 its queued form -- 16 and 32 only together with 8 and never together --, 64 the queued form's
 *            counted twin -- only together with 8 and 32 --, 128 scheduler 1's flows form -- only together with 8, never with 16, 32
 *            or 64 --, 256 the run of the resident form -- only together with 8 and 16, never with 32, 64 or 128.  (8 | 16 | 64 | 256
 *            is the counted run's row of the table: a name without a build, refused.)  A group's build is always of the one-TTI form.
 *   variant  an autotune candidate or a compile-time switch of the batch kernel: extra -D options and / or "ss=<LLVM scheduler
 *            strategy>", space separated; nullptr: none */
struct RsJitSpec {
  int S, U, R, G, NT, sched;
  int qmode = 0, win = 0, flags = 0;
  const char* variant = nullptr;
  /* the LDS carve the build is compiled with: the launch block must carry the same one (rs_jit_launch) */
  RsCarve carve() const { return rs_carve(S, U, R, sched, NT, qmode, win); }
};

struct RsJitKernel;
/* the loaded kernel of this spec on this device, built or read from the disk cache at the first call; nullptr with the reason in err */
extern "C" RsJitKernel* rs_jit_get(int device, const RsJitSpec& spec, char* err, size_t errlen);
extern "C" hipError_t rs_jit_launch(RsJitKernel* k, const RsLaunch* p, hipStream_t stream);
extern "C" int rs_jit_is_untuned(const RsJitKernel* k);  /* built without the -mllvm tuning options (hiprtc refused them) */
extern "C" int rs_jit_is_verified(const RsJitKernel* k); /* carries the self-check mark (this process, or its cache file) */
extern "C" int rs_jit_was_loaded(const RsJitKernel* k);  /* came from the disk cache */
extern "C" void rs_jit_mark_verified(RsJitKernel* k);
extern "C" void rs_jit_reject(RsJitKernel* k);
/* the hiprtc option list of a spec, newline-joined, in `out`; returns its full length.  Not part of the public header: the list is the
 * cache key, and tests/test_jit_option_lists.py holds it to the recorded lists without a GPU. */
extern "C" int rs_jit_option_text(int S, int U, int R, int G, int NT, int sched, int qmode, int win, int flags, const char* variant,
                                  int tuned, char* out, size_t outlen);

#endif /* RS_HOST_H_ */
