"""ctypes binding of include/radiosaber_hip.h.

The classes keep the reference's vocabulary (slices, UEs, RBGs, TTIs):

  SliceConfig      what the reference scheduler constructors read from the JSON config
                   (downlink-transport-scheduler.cpp:55-97): ues_per_slice + per-slice
                   weight / algo_alpha / algo_beta / algo_epsilon / algo_psi
  TtiScheduler     drop-in mode, one RBsAllocation() per call            (rs_create / rs_schedule_tti)
  GroupScheduler   drop-in mode, one TTI of several cells per call       (rs_group_create / rs_group_schedule_tti)
  BatchScheduler   many device-resident cells, whole DoSchedule() loops  (rs_batch_*)
"""
import ctypes as C
import json
import os
from dataclasses import dataclass, field
from pathlib import Path
from typing import List, Optional, Sequence

import numpy as np

RS_SCHED_SUBOPT = 101
RS_SCHED_PF, RS_SCHED_NVS, RS_SCHED_SEQUENTIAL, RS_SCHED_MAXCELL, RS_SCHED_UPPERBOUND, RS_SCHED_NVS_NONGREEDY, RS_SCHED_VOGEL = \
    1, 7, 8, 9, 10, 11, 103

# CQI histogram (CQI 1..15) of the reference's whole cqi-traces-noise0 corpus (158 traces x 475 rows
# x 512 PRBs; SURVEY.md 8d, re-counted by tools/make_trace_fixture.py)
TRACE_CQI_HISTOGRAM = (152600, 56656, 270880, 2088792, 3509504, 1595568, 4145392, 5295816, 1903424,
                       6890232, 4770864, 2842552, 3579624, 96000, 1227696)

_PKG = Path(__file__).resolve().parent
_LIB_PATH = Path(os.environ.get("RS_HIP_LIB", _PKG / "libradiosaber_hip.so"))


class RadioSaberError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"radiosaber_hip error {code}: {msg}")
        self.code = code


class _Config(C.Structure):
    _fields_ = [("n_slices", C.c_int32), ("n_users", C.c_int32), ("n_rbgs", C.c_int32),
                ("rbg_size", C.c_int32), ("sched", C.c_int32), ("device", C.c_int32),
                ("slice_weight", C.POINTER(C.c_double)), ("algo_alpha", C.POINTER(C.c_int32)),
                ("algo_beta", C.POINTER(C.c_int32)), ("algo_epsilon", C.POINTER(C.c_int32)),
                ("algo_psi", C.POINTER(C.c_int32)), ("user_to_slice", C.POINTER(C.c_int32)),
                ("stream", C.c_void_p), ("synthetic_exp", C.c_int32), ("link_tables", C.c_int32)]


class _BatchConfig(C.Structure):
    _fields_ = [("cell", _Config), ("n_cells", C.c_int32), ("first_tti", C.c_int32),
                ("cqi_refresh", C.c_int32), ("phy_error_draws", C.c_int32),
                ("threads_per_cell", C.c_int32), ("jit", C.c_int32),
                ("cqi_epoch_wrap", C.c_int32), ("queue_state_lds", C.c_int32), ("autotune", C.c_int32), ("selfcheck", C.c_int32)]


RS_LINK_DEFAULT, RS_LINK_HOST_LIBM, RS_LINK_PINNED_GLIBC_2_35 = 0, 1, 2  # rs_config.link_tables

RS_ABI_VERSION = 11  # the include/radiosaber_hip.h these ctypes structs mirror; passed to the *_checked create functions


class _TtiIn(C.Structure):
    _fields_ = [("n_users", C.c_int32), ("user_id", C.POINTER(C.c_int32)),
                ("cqi", C.POINTER(C.c_uint8)), ("avg_rate", C.POINTER(C.c_double)),
                ("rand0", C.c_int32), ("rand1", C.c_int32), ("cqi_prb", C.POINTER(C.c_uint8)),
                ("hol_delay", C.POINTER(C.c_double)), ("prio_has_data", C.POINTER(C.c_uint8)),
                ("rand_draws", C.POINTER(C.c_int32)),
                ("required_rbs", C.POINTER(C.c_int32)), ("data_to_transmit", C.POINTER(C.c_int32)), ("cqi_epoch", C.c_uint64)]


class _TtiOut(C.Structure):
    _fields_ = [("target_rbs", C.POINTER(C.c_int32)), ("quota_rbgs", C.POINTER(C.c_int32)),
                ("rbg_to_user", C.POINTER(C.c_int32)), ("user_nprb", C.POINTER(C.c_int32)),
                ("user_final_cqi", C.POINTER(C.c_int32)), ("user_mcs", C.POINTER(C.c_int32)),
                ("user_tbs_bits", C.POINTER(C.c_int32)),
                ("upper_rbg", C.POINTER(C.c_int32)), ("upper_user", C.POINTER(C.c_int32))]


class _BatchLog(C.Structure):
    _fields_ = [("rbg_to_user", C.POINTER(C.c_int16)), ("tbs_bits", C.POINTER(C.c_int32)),
                ("quota", C.POINTER(C.c_int16)), ("target", C.POINTER(C.c_int16)), ("uinfo", C.POINTER(C.c_int32)),
                ("slice_keys", C.POINTER(C.c_uint32))]


class _BatchBearerLog(C.Structure):
    _fields_ = [("bytes", C.POINTER(C.c_int32)), ("hol_delay", C.POINTER(C.c_double))]


# every symbol include/radiosaber_hip.h declares (tests check the library exports all of them)
ABI_SYMBOLS = [
    "rs_last_error", "rs_abi_version", "rs_device_count", "rs_link_tables",
    "rs_create", "rs_destroy", "rs_schedule_tti", "rs_get_slice_offset", "rs_set_slice_offset",
    "rs_batch_create", "rs_batch_destroy", "rs_batch_seed", "rs_batch_upload_cqi_epochs",
    "rs_batch_synthesize_cqi", "rs_batch_download_cqi_epochs", "rs_batch_set_trace",
    "rs_batch_run", "rs_batch_run_async", "rs_batch_sync", "rs_batch_run_logged",
    "rs_batch_run_timed", "rs_batch_read_state", "rs_batch_slice_bytes_device",
    "rs_batch_slice_bytes", "rs_jit_selfcheck", "rs_jit_selfcheck_queue", "rs_batch_debug_stamps", "rs_batch_ttis_done", "rs_batch_stream", "rs_batch_kernel_name",
    "rs_trace_read_mapping", "rs_trace_read_ue_log", "rs_trace_load_dir", "rs_hbm_copy_probe", "rs_lds_bytes_per_cell",
    "rs_get_rbg_size", "rs_dl_prbs_for_bandwidth", "rs_batch_synthesize_cqi_at", "rs_batch_run_logged_ex",
    "rs_batch_read_clock", "rs_batch_jit_status", "rs_batch_prepare_launch",
    "rs_batch_upload_cqi_epochs_prb", "rs_batch_set_trace_prb",
    "rs_batch_set_bearers", "rs_batch_set_arrivals", "rs_batch_read_bearer_state", "rs_internet_flow_arrivals",
    "rs_device_source_hash",
    "rs_create_checked", "rs_batch_create_checked", "rs_jit_selfcheck_untuned", "rs_batch_write_state",
    "rs_ctx_specialize", "rs_jit_selfcheck_dropin",
    "rs_batch_debug_heap_sorts", "rs_ctx_debug_heap_sorts",
    "rs_jit_cache_stats", "rs_jit_cache_file", "rs_jit_cache_warm", "rs_batch_autotune_report", "rs_batch_debug_clocks",
    "rs_batch_checkpoint_bytes", "rs_batch_checkpoint_save", "rs_batch_checkpoint_load",
    "rs_link_tables_pinned", "rs_link_tables_compare", "rs_ctx_jit_status", "rs_jit_compiler_identity",
    "rs_batch_flow_record", "rs_batch_run_logged_bearers",
    "rs_group_create", "rs_group_create_checked", "rs_group_destroy", "rs_group_schedule_tti",
    "rs_group_get_slice_offset", "rs_group_set_slice_offset", "rs_group_launch_count", "rs_group_kernel_name",
    "rs_group_image_stats", "rs_group_specialize", "rs_group_jit_status", "rs_jit_selfcheck_group",
    "rs_group_set_avg", "rs_group_get_avg", "rs_group_set_pending", "rs_group_schedule_tti_at", "rs_group_run_at",
    "rs_group_specialize_resident", "rs_group_resident_jit_status", "rs_jit_selfcheck_group_resident",
    "rs_group_set_bearers", "rs_group_get_bearers", "rs_group_schedule_tti_queued",
    "rs_group_specialize_queued", "rs_group_queued_jit_status", "rs_jit_selfcheck_group_queued",
    "rs_group_set_counters", "rs_group_get_counters", "rs_group_schedule_tti_counted",
    "rs_group_set_flows", "rs_group_get_flows", "rs_group_schedule_tti_flows",
    "rs_group_specialize_counted", "rs_group_counted_jit_status", "rs_jit_selfcheck_group_counted",
    "rs_group_specialize_flows", "rs_group_flows_jit_status", "rs_jit_selfcheck_group_flows",
    "rs_group_specialize_run", "rs_group_run_jit_status", "rs_jit_selfcheck_group_run",
    "rs_group_set_avg_counters", "rs_group_get_avg_counters", "rs_group_run_counted_at",
    "rs_group_grant_bound", "rs_group_run_records_at",
    "rs_batch_record_bound", "rs_batch_run_records",
]

# rs_grant_record: one grant of one TTI of a counted run (32 bytes)
GRANT_RECORD = np.dtype([("pos", np.int32), ("user_id", np.int32), ("bytes", np.int32), ("nprb", np.int32),
                         ("cum_bytes", np.int64), ("cum_rbs", np.int64)])
assert GRANT_RECORD.itemsize == 32
# rs_bearer_record: one bearer that DoStopSchedule credited in one TTI of a queue-model batch (32 bytes)
BEARER_RECORD = np.dtype([("tti", np.int32), ("user", np.int32), ("bearer", np.int32), ("bytes", np.int32), ("nprb", np.int32),
                          ("reserved", np.int32), ("hol_delay", np.float64)])
assert BEARER_RECORD.itemsize == 32

_lib = None


def lib():
    """Load libradiosaber_hip.so (fails loudly when it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not _LIB_PATH.exists():
        raise RadioSaberError(-100, f"{_LIB_PATH} is missing: run `python -m radiosaber_amd.build` "
                                    "(there is no CPU fallback)")
    L = C.CDLL(str(_LIB_PATH))
    L.rs_last_error.restype = C.c_char_p
    L.rs_link_tables.argtypes = [C.POINTER(C.c_double)] * 4
    L.rs_link_tables_pinned.argtypes = [C.POINTER(C.c_double)] * 4
    L.rs_link_tables_compare.argtypes = [C.c_char_p, C.c_size_t]
    L.rs_ctx_jit_status.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.rs_jit_compiler_identity.restype = C.c_char_p
    L.rs_jit_compiler_identity.argtypes = []
    L.rs_create.restype = C.c_void_p
    L.rs_create.argtypes = [C.POINTER(_Config)]
    L.rs_destroy.argtypes = [C.c_void_p]
    L.rs_schedule_tti.argtypes = [C.c_void_p, C.POINTER(_TtiIn), C.POINTER(_TtiOut)]
    L.rs_get_slice_offset.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.rs_set_slice_offset.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.rs_group_create.restype = C.c_void_p
    L.rs_group_create.argtypes = [C.POINTER(_Config), C.c_int32]
    L.rs_group_create_checked.restype = C.c_void_p
    L.rs_group_create_checked.argtypes = [C.POINTER(_Config), C.c_int32, C.c_int, C.c_size_t]
    L.rs_group_destroy.argtypes = [C.c_void_p]
    L.rs_group_schedule_tti.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(_TtiIn), C.POINTER(_TtiOut)]
    L.rs_group_get_slice_offset.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_double)]
    L.rs_group_set_slice_offset.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_double)]
    L.rs_group_launch_count.restype = C.c_int64
    L.rs_group_launch_count.argtypes = [C.c_void_p]
    L.rs_group_image_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    L.rs_group_kernel_name.restype = C.c_char_p
    L.rs_group_kernel_name.argtypes = [C.c_void_p]
    L.rs_group_specialize.argtypes = [C.c_void_p]
    L.rs_group_set_avg.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.c_double]
    L.rs_group_get_avg.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    L.rs_group_set_pending.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
    L.rs_group_schedule_tti_at.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(_TtiIn), C.POINTER(_TtiOut), C.POINTER(C.c_double)]
    L.rs_group_run_at.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(_TtiIn), C.c_int32, C.POINTER(C.c_double),
                                  C.POINTER(C.c_int32), C.POINTER(_TtiOut)]
    L.rs_group_set_bearers.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_uint8), C.POINTER(C.c_double), C.c_double]
    L.rs_group_get_bearers.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    L.rs_group_schedule_tti_queued.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(_TtiIn), C.POINTER(_TtiOut),
                                               C.POINTER(C.c_double), C.POINTER(C.POINTER(C.c_int32))]
    L.rs_group_jit_status.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.rs_jit_selfcheck_group.argtypes = [C.c_int] * 6 + [C.c_char_p, C.c_size_t]
    L.rs_group_specialize_resident.argtypes = [C.c_void_p]
    L.rs_group_resident_jit_status.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.rs_jit_selfcheck_group_resident.argtypes = [C.c_int] * 6 + [C.c_char_p, C.c_size_t]
    L.rs_group_set_counters.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.rs_group_set_avg_counters.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.rs_group_get_avg_counters.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.rs_group_run_counted_at.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(_TtiIn), C.c_int32, C.POINTER(C.c_double),
                                          C.POINTER(C.c_int32), C.POINTER(_TtiOut)]
    L.rs_group_grant_bound.argtypes = [C.c_void_p]
    L.rs_group_run_records_at.argtypes = L.rs_group_run_counted_at.argtypes + [C.c_int32, C.c_void_p, C.POINTER(C.c_int32)]
    L.rs_group_get_counters.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.rs_group_schedule_tti_counted.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(_TtiIn), C.POINTER(_TtiOut),
                                                C.POINTER(C.c_double), C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.POINTER(C.c_int32))]
    L.rs_group_set_flows.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_uint8), C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_int64),
                                     C.POINTER(C.c_int64)]
    L.rs_group_get_flows.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                     C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.rs_group_schedule_tti_flows.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(_TtiIn), C.POINTER(_TtiOut),
                                              C.POINTER(C.c_double), C.POINTER(C.POINTER(C.c_uint8))]
    L.rs_group_specialize_queued.argtypes = [C.c_void_p]
    L.rs_group_queued_jit_status.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.rs_jit_selfcheck_group_queued.argtypes = [C.c_int] * 6 + [C.c_char_p, C.c_size_t]
    L.rs_group_specialize_counted.argtypes = [C.c_void_p]
    L.rs_group_counted_jit_status.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.rs_jit_selfcheck_group_counted.argtypes = [C.c_int] * 6 + [C.c_char_p, C.c_size_t]
    L.rs_group_specialize_flows.argtypes = [C.c_void_p]
    L.rs_group_flows_jit_status.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.rs_jit_selfcheck_group_flows.argtypes = [C.c_int] * 6 + [C.c_char_p, C.c_size_t]
    L.rs_group_specialize_run.argtypes = [C.c_void_p]
    L.rs_group_run_jit_status.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.rs_jit_selfcheck_group_run.argtypes = [C.c_int] * 6 + [C.c_char_p, C.c_size_t]
    L.rs_batch_create.restype = C.c_void_p
    L.rs_batch_create.argtypes = [C.POINTER(_BatchConfig)]
    L.rs_create_checked.restype = C.c_void_p
    L.rs_create_checked.argtypes = [C.POINTER(_Config), C.c_int, C.c_size_t]
    L.rs_batch_create_checked.restype = C.c_void_p
    L.rs_batch_create_checked.argtypes = [C.POINTER(_BatchConfig), C.c_int, C.c_size_t]
    L.rs_jit_selfcheck_untuned.argtypes = [C.c_int] * 6 + [C.c_char_p, C.c_size_t]
    L.rs_jit_selfcheck_dropin.argtypes = [C.c_int] * 6 + [C.c_char_p, C.c_size_t]
    L.rs_ctx_specialize.argtypes = [C.c_void_p]
    L.rs_batch_destroy.argtypes = [C.c_void_p]
    L.rs_batch_seed.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_int64)]
    L.rs_batch_upload_cqi_epochs.argtypes = [C.c_void_p, C.POINTER(C.c_uint8), C.c_int32]
    L.rs_batch_synthesize_cqi.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_double), C.c_int32]
    L.rs_batch_synthesize_cqi_at.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_double), C.c_int32, C.c_int64]
    L.rs_batch_run_logged_ex.argtypes = [C.c_void_p, C.c_int32, C.POINTER(_BatchLog)]
    L.rs_batch_run_logged_bearers.argtypes = [C.c_void_p, C.c_int32, C.POINTER(_BatchLog), C.POINTER(_BatchBearerLog)]
    L.rs_batch_flow_record.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    L.rs_batch_record_bound.argtypes = [C.c_void_p]
    L.rs_batch_run_records.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.POINTER(C.c_int64)]
    L.rs_batch_read_clock.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.rs_batch_jit_status.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.rs_batch_prepare_launch.argtypes = [C.c_void_p, C.c_int32]
    L.rs_batch_upload_cqi_epochs_prb.argtypes = [C.c_void_p, C.POINTER(C.c_uint8), C.c_int32]
    L.rs_batch_set_trace_prb.argtypes = [C.c_void_p, C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
    L.rs_batch_set_bearers.argtypes = [C.c_void_p, C.POINTER(C.c_uint8)]
    L.rs_batch_set_arrivals.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_int32),
                                        C.POINTER(C.c_int32)]
    L.rs_batch_read_bearer_state.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                             C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.rs_internet_flow_arrivals.argtypes = [C.c_double, C.c_double, C.c_double, C.c_uint32, C.c_int32, C.POINTER(C.c_double),
                                            C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.rs_get_rbg_size.argtypes = [C.c_int]
    L.rs_dl_prbs_for_bandwidth.argtypes = [C.c_double]
    L.rs_batch_download_cqi_epochs.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_uint8)]
    L.rs_batch_set_trace.argtypes = [C.c_void_p, C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32,
                                     C.POINTER(C.c_int32)]
    L.rs_batch_run.argtypes = [C.c_void_p, C.c_int32]
    L.rs_batch_run_async.argtypes = [C.c_void_p, C.c_int32]
    L.rs_batch_sync.argtypes = [C.c_void_p]
    L.rs_batch_run_logged.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int16), C.POINTER(C.c_int32),
                                      C.POINTER(C.c_int16), C.POINTER(C.c_int16), C.POINTER(C.c_int32)]
    L.rs_batch_run_timed.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_float)]
    L.rs_batch_read_state.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                      C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    L.rs_batch_write_state.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.rs_batch_slice_bytes_device.argtypes = [C.c_void_p, C.c_void_p]
    L.rs_batch_slice_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.rs_jit_selfcheck.argtypes = [C.c_int] * 6 + [C.c_char_p, C.c_size_t]
    L.rs_jit_selfcheck_queue.argtypes = [C.c_int] * 6 + [C.c_char_p, C.c_size_t]
    L.rs_batch_debug_stamps.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_uint64)]
    L.rs_batch_debug_heap_sorts.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    L.rs_ctx_debug_heap_sorts.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    L.rs_jit_cache_stats.argtypes = [C.POINTER(C.c_longlong)]
    L.rs_jit_cache_stats.restype = None
    L.rs_jit_cache_file.argtypes = [C.c_int] * 7 + [C.c_char_p, C.c_size_t]
    L.rs_jit_cache_warm.argtypes = [C.c_int] * 7 + [C.c_char_p, C.c_size_t]
    L.rs_batch_autotune_report.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.rs_batch_debug_clocks.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.rs_batch_checkpoint_bytes.restype = C.c_int64
    L.rs_batch_checkpoint_bytes.argtypes = [C.c_void_p]
    L.rs_batch_checkpoint_save.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.rs_batch_checkpoint_load.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.rs_batch_ttis_done.restype = C.c_int64
    L.rs_batch_ttis_done.argtypes = [C.c_void_p]
    L.rs_batch_stream.restype = C.c_void_p
    L.rs_batch_stream.argtypes = [C.c_void_p]
    L.rs_batch_kernel_name.restype = C.c_char_p
    L.rs_batch_kernel_name.argtypes = [C.c_void_p]
    L.rs_lds_bytes_per_cell.argtypes = [C.c_int] * 5
    L.rs_device_source_hash.restype = C.c_char_p
    L.rs_device_source_hash.argtypes = []
    L.rs_hbm_copy_probe.argtypes = [C.c_int, C.c_uint64, C.c_int, C.POINTER(C.c_double)]
    L.rs_trace_read_mapping.argtypes = [C.c_char_p, C.POINTER(C.c_int32), C.c_int32]
    L.rs_trace_read_ue_log.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8),
                                       C.POINTER(C.c_uint8)]
    L.rs_trace_load_dir.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8)]
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise RadioSaberError(rc, lib().rs_last_error().decode())


def _count(rc):
    """calls that return a count (>= 0) or a negative RS_ERR_*"""
    if rc < 0:
        raise RadioSaberError(rc, lib().rs_last_error().decode())
    return rc


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def jit_selfcheck(n_slices, n_users, n_rbgs, rbg_size, threads=512, sched=RS_SCHED_MAXCELL, queues=False, untuned=False, dropin=False,
                  group=False, resident=False, queued=False, counted=False, flows=False, run=False):
    """Compile the shape-specialised kernel for one shape (hiprtc, no GPU needed); returns the code size.  queues=True: the
    queue-model kernel of the shape.  untuned=True: without the -mllvm tuning options (the library's fallback build).
    group=True: the general and the lean build of a group of this shape (rs_group_specialize); the larger code size.
    group=True, resident=True: the two builds of the group's resident kernel (rs_group_specialize_resident).
    group=True, queued=True: the two builds of the group's queued kernel (rs_group_specialize_queued; schedulers 7, 8, 9, 101, 103).
    group=True, counted=True: the two builds of the group's counted kernel (rs_group_specialize_counted; the queued form's schedulers).
    group=True, flows=True: the two builds of the group's flows kernel (rs_group_specialize_flows; scheduler 1).
    group=True, resident=True, run=True: the two builds of the group's run kernel (rs_group_specialize_run; never schedulers 7 and 11)."""
    _jit_flags(False, False, group, resident, queued, counted, flows, run)
    buf = C.create_string_buffer(4096)
    fn = lib().rs_jit_selfcheck_queue if queues else (lib().rs_jit_selfcheck_untuned if untuned else lib().rs_jit_selfcheck)
    if dropin:  # the drop-in entry point's one-TTI kernel of a context of this shape (rs_ctx_specialize)
        fn = lib().rs_jit_selfcheck_dropin
    if group:
        fn = lib().rs_jit_selfcheck_group_resident if resident else lib().rs_jit_selfcheck_group
        if queued:
            fn = lib().rs_jit_selfcheck_group_queued
        if counted:
            fn = lib().rs_jit_selfcheck_group_counted
        if flows:
            fn = lib().rs_jit_selfcheck_group_flows
        if run:
            fn = lib().rs_jit_selfcheck_group_run
    n = fn(n_slices, n_users, n_rbgs, rbg_size, threads, sched, buf, 4096)
    if n < 0:
        raise RadioSaberError(n, buf.value.decode(errors="replace"))
    return n


def jit_cache_stats():
    """This process's disk-cache counters of the run-time compiled kernels: dict(hits, misses, stores, rejected)."""
    out = (C.c_longlong * 4)()
    lib().rs_jit_cache_stats(out)
    return dict(zip(("hits", "misses", "stores", "rejected"), (int(x) for x in out)))


def _jit_flags(lean, streamed, group, resident, queued=False, counted=False, flows=False, run=False):
    if run and not (group and resident):
        raise ValueError("run=True needs group=True and resident=True: the run kernel is the resident form's")
    if run and (queued or counted or flows):
        raise ValueError("run=True excludes queued=True, counted=True and flows=True: only the resident form has a run")
    if counted and not group:
        raise ValueError("counted=True needs group=True: only a group has a counted kernel")
    if flows and not group:
        raise ValueError("flows=True needs group=True: only a group has a flows kernel")
    if counted and resident:
        raise ValueError("resident=True and counted=True exclude each other: two forms of a group's kernel")
    if flows and (resident or queued or counted):
        raise ValueError("flows=True excludes resident=True, queued=True and counted=True: a form of a group's kernel of its own")
    if counted:
        queued = True  # (the counted form is the queued form's twin: flag value 64 is valid only together with 32)
    if resident and not group:
        raise ValueError("resident=True needs group=True: only a group has a resident kernel")
    if queued and not group:
        raise ValueError("queued=True needs group=True: only a group has a queued kernel")
    if queued and resident:
        raise ValueError("resident=True and queued=True exclude each other: two forms of a group's kernel")
    return (4 if lean else 0) | (2 if streamed else 0) | (8 if group else 0) | (16 if resident else 0) | (32 if queued else 0) | \
        (64 if counted else 0) | (128 if flows else 0) | (256 if run else 0)


def jit_cache_file(n_slices, n_users, n_rbgs, rbg_size, threads=512, sched=RS_SCHED_MAXCELL, lean=False, streamed=False, group=False,
                   resident=False, queued=False, counted=False, flows=False, run=False):
    """Path of the cache file the batch kernel of this shape lives in ('' when no cache directory can be named).  group=True: a
    group's build of the one-TTI kernel (flag bit of value 8); with resident=True its resident form (value 16), with queued=True its
    queued form (value 32), with counted=True the queued form's counted twin (values 32 and 64), with flows=True scheduler 1's flows form
    (value 128), with resident=True and run=True the resident form's run (values 16 and 256)."""
    buf = C.create_string_buffer(4096)
    lib().rs_jit_cache_file(n_slices, n_users, n_rbgs, rbg_size, threads, sched, _jit_flags(lean, streamed, group, resident, queued, counted, flows, run),
                            buf, 4096)
    return buf.value.decode()


def jit_cache_warm(n_slices, n_users, n_rbgs, rbg_size, threads=512, sched=RS_SCHED_MAXCELL, lean=False, streamed=False, group=False,
                   resident=False, queued=False, counted=False, flows=False, run=False):
    """Compile (or load) the batch kernel of this shape through the disk cache; no GPU needed.  Returns the code size.
    group=True: a group's build of the one-TTI kernel; with resident=True its resident form, with queued=True its queued form, with
    counted=True its counted form, with flows=True its flows form, with resident=True and run=True the resident form's run."""
    buf = C.create_string_buffer(4096)
    n = lib().rs_jit_cache_warm(n_slices, n_users, n_rbgs, rbg_size, threads, sched, _jit_flags(lean, streamed, group, resident, queued, counted, flows, run),
                                buf, 4096)
    if n < 0:
        raise RadioSaberError(n, buf.value.decode(errors="replace"))
    return n


def device_count():
    return lib().rs_device_count()


def device_source_hash():
    """Identity of the device code inside the library (FNV-1a of the embedded kernel sources, 16 hex digits)."""
    return lib().rs_device_source_hash().decode()


def get_rbg_size(nb_rbs):
    """PRBs per RBG (ref: src/utility/eesm-effective-sinr.h:82-103); raises above 512 PRBs like the reference throws."""
    return _count(lib().rs_get_rbg_size(nb_rbs))


def dl_prbs_for_bandwidth(bw_mhz):
    """PRBs of a downlink bandwidth in MHz (ref: src/core/spectrum/bandwidth-manager.cpp:30-38, 52-108)."""
    return lib().rs_dl_prbs_for_bandwidth(float(bw_mhz))


BEARER_NONE, BEARER_BACKLOG, BEARER_QUEUE = 0, 1, 2
FULL_PACKET = 1495  # MAXMTUSIZE 1490 + UDP 8 + IP 20, ROHC 28 -> 3, PDCP 2 (ref: src/protocolStack/packet/Packet.cpp:84-118)


def internet_flow_arrivals(rate_mbps, start_time, stop_time, size_seed, max_bursts=1 << 16):
    """Arrival bursts of one InternetFlow application (ref: src/flows/application/InternetFlow.cpp): (time f64[n], n_full i32[n],
    last_bytes i32[n]); no GPU needed."""
    t = np.zeros(max_bursts, np.float64)
    nf = np.zeros(max_bursts, np.int32)
    la = np.zeros(max_bursts, np.int32)
    n = _count(lib().rs_internet_flow_arrivals(rate_mbps, start_time, stop_time, size_seed, max_bursts, _p(t, C.c_double),
                                               _p(nf, C.c_int32), _p(la, C.c_int32)))
    return t[:n].copy(), nf[:n].copy(), la[:n].copy()


def frames_to_bursts(times, frame_bytes, mtu=1490):
    """Frames of a video trace as arrival bursts (ref: src/flows/application/TraceBased.cpp:155-224): size/1490 packets of
    1490 + 5 bytes and, for a remainder, one of remainder + 5 bytes (this application adds the headers to the last packet too)."""
    fb = np.asarray(frame_bytes, np.int64)
    rem = fb % mtu
    return (np.ascontiguousarray(times, np.float64), (fb // mtu).astype(np.int32),
            np.where(rem > 0, rem + (FULL_PACKET - mtu), 0).astype(np.int32))


def lds_bytes_per_cell(n_slices, n_users, n_rbgs, sched=RS_SCHED_MAXCELL, threads=512):
    """LDS bytes of one cell of this shape (<= 40 960: four cells per CU, <= 81 920: two)."""
    return _count(lib().rs_lds_bytes_per_cell(n_slices, n_users, n_rbgs, sched, threads))


def hbm_copy_probe(device=0, nbytes=1 << 30, iters=10):
    """GB/s of a 16 B/lane streaming copy (read + write bytes over time) -- the attainable HBM rate."""
    g = C.c_double(0)
    _check(lib().rs_hbm_copy_probe(device, nbytes, iters, C.byref(g)))
    return g.value


def link_tables(pinned=False):
    """Link adaptation tables (no GPU needed): dict of eff/kbps/E/X, each float64[16] -- as this host's libm evaluates them, or
    (pinned=True) the glibc-2.35 set compiled into the library (rs_config.link_tables)."""
    out = [np.zeros(16, np.float64) for _ in range(4)]
    _check((lib().rs_link_tables_pinned if pinned else lib().rs_link_tables)(*[_p(a, C.c_double) for a in out]))
    return dict(zip(("eff", "kbps", "eesm_e", "eesm_x"), out))


def link_tables_compare():
    """(n, text): how many EESM constants of this host's libm differ from the pinned glibc-2.35 set, and which."""
    buf = C.create_string_buffer(4096)
    return _count(lib().rs_link_tables_compare(buf, 4096)), buf.value.decode(errors="replace")


def jit_compiler_identity():
    """The compiler identity inside every cache key of the run-time builds (hiprtc / HIP runtime / clang with its LLVM commit / comgr)."""
    return lib().rs_jit_compiler_identity().decode()


def read_trace_mapping(path, max_entries=4096):
    """mapping<i>.config of the reference's cqi-traces-noise0 -> int32[n]: user u replays trace map[u % n]
    (ref: enb-mac-entity.cc:47-53, :171)."""
    out = np.zeros(max_entries, dtype=np.int32)
    n = _count(lib().rs_trace_read_mapping(os.fsencode(str(path)), _p(out, C.c_int32), max_entries))
    if n > max_entries:
        raise RadioSaberError(-1, f"{path}: {n} entries, max_entries={max_entries}")
    return out[:n].copy()


def read_ue_trace(path, nb_rbs=512, rbg_size=8, n_rows=475, per_prb=False):
    """One ue<id>.log -> (uint8[n_rows][nb_rbs/rbg_size], mixed) or, per_prb=True, (uint8[n_rows][nb_rbs], mixed);
    `mixed` counts RBGs whose PRBs differ (0: the RBG-granular replay is exact).  ref: enb-mac-entity.cc:173-186."""
    R = nb_rbs // rbg_size
    rbg = np.zeros((n_rows, R), dtype=np.uint8)
    prb = np.zeros((n_rows, nb_rbs), dtype=np.uint8) if per_prb else None
    rc = _count(lib().rs_trace_read_ue_log(os.fsencode(str(path)), n_rows, nb_rbs, rbg_size, _p(rbg, C.c_uint8),
                                           _p(prb, C.c_uint8) if per_prb else None))
    return (prb if per_prb else rbg), rc


def load_trace_dir(directory, n_traces=158, nb_rbs=512, rbg_size=8, n_rows=475):
    """ue0.log .. ue<n_traces-1>.log -> (uint8[n_traces][n_rows][R], mixed): the `trace` argument of
    BatchScheduler.set_trace (MAX_UE_TRACE = 158, MAX_TTI_TRACE = 475 in the reference)."""
    R = nb_rbs // rbg_size
    out = np.zeros((n_traces, n_rows, R), dtype=np.uint8)
    rc = _count(lib().rs_trace_load_dir(os.fsencode(str(directory)), n_traces, n_rows, nb_rbs, rbg_size,
                                        _p(out, C.c_uint8)))
    return out, rc


@dataclass
class SliceConfig:
    """The reference's JSON scheduler config (downlink-transport-scheduler.cpp:65-88;
    single-cell-with-interference.h:220-248): `slices` groups expand in order."""
    ues_per_slice: List[int]
    weight: List[float] = field(default_factory=list)
    algo_alpha: List[int] = field(default_factory=list)
    algo_beta: List[int] = field(default_factory=list)
    algo_epsilon: List[int] = field(default_factory=list)
    algo_psi: List[int] = field(default_factory=list)
    # per slice, what every UE of the slice runs (single-cell-with-interference.h:226-248, 300-440): {"backlog_flow": n,
    # "internet_flow": n, "if_bitrate": [Mbps per slice, ...], "video_app": n, "video_bitrate": [kbps, ...]}; empty = one
    # InfiniteBuffer flow per UE
    traffic: List[dict] = field(default_factory=list)

    def __post_init__(self):
        S = len(self.ues_per_slice)
        if not self.weight:
            self.weight = [1.0 / S] * S
        for name, default in (("algo_alpha", 0), ("algo_beta", 0), ("algo_epsilon", 1), ("algo_psi", 1)):
            if not getattr(self, name):
                setattr(self, name, [default] * S)
        for name in ("weight", "algo_alpha", "algo_beta", "algo_epsilon", "algo_psi"):
            if len(getattr(self, name)) != S:
                raise ValueError(f"{name} has {len(getattr(self, name))} entries for {S} slices")

    @classmethod
    def from_json(cls, path_or_dict):
        obj = path_or_dict if isinstance(path_or_dict, dict) else json.loads(Path(path_or_dict).read_text())
        ues = [int(x) for x in obj["ues_per_slice"]]
        w, a, b, e, p, tr = [], [], [], [], [], []
        for grp in obj["slices"]:
            for _ in range(int(grp["n_slices"])):
                w.append(float(grp["weight"]))
                a.append(int(grp.get("algo_alpha", 0)))
                b.append(int(grp.get("algo_beta", 0)))
                e.append(int(grp.get("algo_epsilon", 0)))
                p.append(int(grp.get("algo_psi", 0)))
                tr.append({k: grp[k] for k in ("backlog_flow", "internet_flow", "if_bitrate", "video_app", "video_bitrate")
                           if k in grp})
        return cls(ues, w, a, b, e, p, tr if any(tr) else [])

    def bearer_kinds(self):
        """[U][2] bearer kinds (index = priority) from `traffic`: InternetFlow j has priority j, every other application
        priority 0 (RadioBearer::GetPriority, src/flows/radio-bearer.cpp:88-97)."""
        k = np.zeros((self.n_users, 2), np.uint8)
        u2s = self.user_to_slice
        for u in range(self.n_users):
            t = self.traffic[u2s[u]] if self.traffic else {}
            nif = int(t.get("internet_flow", 0))
            if nif > 2:
                raise ValueError("more than MAX_BEARERS = 2 internet flows per UE")
            for j in range(nif):
                k[u, j] = BEARER_QUEUE
            if int(t.get("video_app", 0)) and not nif:
                k[u, 0] = BEARER_QUEUE
            if (int(t.get("backlog_flow", 0)) or not t) and not k[u, 0]:
                k[u, 0] = BEARER_BACKLOG
        return k

    @property
    def n_slices(self):
        return len(self.ues_per_slice)

    @property
    def n_users(self):
        return int(sum(self.ues_per_slice))

    @property
    def user_to_slice(self):
        return np.repeat(np.arange(self.n_slices, dtype=np.int32), self.ues_per_slice).astype(np.int32)


class _CfgHolder:
    """Keeps the numpy arrays a C rs_config points at alive."""

    def __init__(self, slices: SliceConfig, n_rbgs, rbg_size, sched, device, stream, synthetic_exp=False, link_tables=0):
        self.w = np.ascontiguousarray(slices.weight, np.float64)
        self.a = np.ascontiguousarray(slices.algo_alpha, np.int32)
        self.b = np.ascontiguousarray(slices.algo_beta, np.int32)
        self.e = np.ascontiguousarray(slices.algo_epsilon, np.int32)
        self.p = np.ascontiguousarray(slices.algo_psi, np.int32)
        self.u2s = np.ascontiguousarray(slices.user_to_slice, np.int32)
        self.c = _Config(slices.n_slices, slices.n_users, n_rbgs, rbg_size, sched, device,
                         _p(self.w, C.c_double), _p(self.a, C.c_int32), _p(self.b, C.c_int32),
                         _p(self.e, C.c_int32), _p(self.p, C.c_int32), _p(self.u2s, C.c_int32),
                         C.c_void_p(stream or 0), int(bool(synthetic_exp)), int(link_tables))


@dataclass
class TtiResult:
    target_rbs: np.ndarray
    quota_rbgs: np.ndarray
    rbg_to_user: np.ndarray
    user_nprb: np.ndarray
    user_final_cqi: np.ndarray
    user_mcs: np.ndarray
    user_tbs_bits: np.ndarray
    upper_rbg: Optional[np.ndarray] = None   # RS_SCHED_UPPERBOUND: [S][R] RBGs each slice took, push order, -1 padded
    upper_user: Optional[np.ndarray] = None  # ... and the user each one went to
    sent: Optional[np.ndarray] = None        # GroupScheduler.schedule_tti_counted: [n][2] bytes DoStopSchedule sent per call position and bearer


def _marshal_tti(S, R, rbg_size, sched, cqi, avg_rate, rand0=0, rand1=0, user_id=None, cqi_prb=None, hol_delay=None, prio_has_data=None,
                 rand_draws=None, required_rbs=None, data_to_transmit=None, cqi_epoch=0):
    """One call's arguments as (rs_tti_in, rs_tti_out, TtiResult, the arrays the two structs point at)."""
    prb = None
    if cqi_prb is not None:
        prb = np.ascontiguousarray(cqi_prb, np.uint8)
        n = prb.shape[0]
        assert prb.shape == (n, R * rbg_size)
        cqi = None
    else:
        cqi = np.ascontiguousarray(cqi, np.uint8)
        n = cqi.shape[0]
        assert cqi.shape == (n, R)
    avg = None if avg_rate is None else np.ascontiguousarray(avg_rate, np.float64)  # (None: a resident call, GroupScheduler.schedule_tti_at)
    assert avg is None or avg.shape == (n,)
    uid = None if user_id is None else np.ascontiguousarray(user_id, np.int32)
    hol = None if hol_delay is None else np.ascontiguousarray(hol_delay, np.float64)
    prio = None if prio_has_data is None else np.ascontiguousarray(prio_has_data, np.uint8)
    draws = None if rand_draws is None else np.ascontiguousarray(rand_draws, np.int32)
    assert draws is None or draws.size == 300 * n
    req = None if required_rbs is None else np.ascontiguousarray(required_rbs, np.int32)
    dat = None if data_to_transmit is None else np.ascontiguousarray(data_to_transmit, np.int32)
    assert (req is None or req.shape == (n,)) and (dat is None or dat.shape == (n,))
    res = TtiResult(np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(R, np.int32),
                    np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32))
    tin = _TtiIn(n, _p(uid, C.c_int32) if uid is not None else None,
                 _p(cqi, C.c_uint8) if cqi is not None else None, _p(avg, C.c_double) if avg is not None else None, rand0, rand1,
                 _p(prb, C.c_uint8) if prb is not None else None,
                 _p(hol, C.c_double) if hol is not None else None,
                 _p(prio, C.c_uint8) if prio is not None else None,
                 _p(draws, C.c_int32) if draws is not None else None,
                 _p(req, C.c_int32) if req is not None else None,
                 _p(dat, C.c_int32) if dat is not None else None, int(cqi_epoch))
    if sched == RS_SCHED_UPPERBOUND:
        res.upper_rbg = np.full((S, R), -1, np.int32)
        res.upper_user = np.full((S, R), -1, np.int32)
    tout = _TtiOut(_p(res.target_rbs, C.c_int32), _p(res.quota_rbgs, C.c_int32),
                   _p(res.rbg_to_user, C.c_int32), _p(res.user_nprb, C.c_int32),
                   _p(res.user_final_cqi, C.c_int32), _p(res.user_mcs, C.c_int32),
                   _p(res.user_tbs_bits, C.c_int32),
                   _p(res.upper_rbg, C.c_int32) if res.upper_rbg is not None else None,
                   _p(res.upper_user, C.c_int32) if res.upper_user is not None else None)
    return tin, tout, res, (cqi, prb, avg, uid, hol, prio, draws, req, dat)


class TtiScheduler:
    """Drop-in mode: RBsAllocation() of one TTI on the GPU (rs_create / rs_schedule_tti)."""

    def __init__(self, slices: SliceConfig, n_rbgs: int, rbg_size: int, sched: int = RS_SCHED_MAXCELL,
                 device: int = 0, stream: Optional[int] = None, synthetic_exp: bool = False, jit: bool = False,
                 link_tables: int = RS_LINK_DEFAULT):
        """jit: rs_ctx_specialize -- this context's own hiprtc build of the one-TTI kernel (identical results, shorter calls; its first
        calls run beside the built-in kernel unless the build carries the self-check mark: jit_status()).
        link_tables: RS_LINK_* (default for a drop-in context: this host's libm; create_warning says when it is not the fixtures')."""
        self.slices, self.R, self.rbg_size, self.sched = slices, n_rbgs, rbg_size, sched
        self._cfg = _CfgHolder(slices, n_rbgs, rbg_size, sched, device, stream, synthetic_exp, link_tables)
        self._h = lib().rs_create_checked(C.byref(self._cfg.c), RS_ABI_VERSION, C.sizeof(_Config))
        if not self._h:
            raise RadioSaberError(-1, lib().rs_last_error().decode())
        self.create_warning = lib().rs_last_error().decode()
        if jit:
            _check(lib().rs_ctx_specialize(self._h))

    def jit_status(self):
        """(code, message) of rs_ctx_jit_status: 1 specialised kernels serve, 0 not asked for, -1 build failed, -2 dropped by the self-check."""
        buf = C.create_string_buffer(512)
        rc = lib().rs_ctx_jit_status(self._h, buf, 512)
        return rc, buf.value.decode(errors="replace")

    def close(self):
        if getattr(self, "_h", None):
            lib().rs_destroy(self._h)
            self._h = None

    __del__ = close

    def schedule_tti(self, cqi, avg_rate, rand0=0, rand1=0, user_id: Optional[Sequence[int]] = None,
                     cqi_prb=None, hol_delay=None, prio_has_data=None, rand_draws=None, required_rbs=None,
                     data_to_transmit=None, cqi_epoch: int = 0) -> TtiResult:
        """cqi [n][R] per-RBG CQI, or cqi_prb [n][R*rbg_size] per-PRB CQI (then cqi may be None).
        rand_draws (RS_SCHED_NVS_NONGREEDY): the 300 * n rand() values of RBsAllocationNonGreedyPF, in draw order.
        cqi_epoch: non-zero = the caller's version number of the CQI block; a call with the number (and users) of the call before reads
        the context's device-resident image instead of the block (rs_tti_in.cqi_epoch)."""
        tin, tout, res, _keep = _marshal_tti(self.slices.n_slices, self.R, self.rbg_size, self.sched, cqi, avg_rate, rand0, rand1, user_id,
                                             cqi_prb, hol_delay, prio_has_data, rand_draws, required_rbs, data_to_transmit, cqi_epoch)
        _check(lib().rs_schedule_tti(self._h, C.byref(tin), C.byref(tout)))
        return res

    def heap_sorts(self):
        """int64[3]: heap-sort fallbacks of the std::sort emulation so far, per device site (rs_ctx_debug_heap_sorts)."""
        out = np.zeros(3, np.int64)
        _check(lib().rs_ctx_debug_heap_sorts(self._h, _p(out, C.c_int64)))
        return out

    @property
    def slice_offset(self):
        out = np.zeros(self.slices.n_slices, np.float64)
        _check(lib().rs_get_slice_offset(self._h, _p(out, C.c_double)))
        return out

    @slice_offset.setter
    def slice_offset(self, v):
        a = np.ascontiguousarray(v, np.float64)
        _check(lib().rs_set_slice_offset(self._h, _p(a, C.c_double)))


class GroupScheduler:
    """Drop-in mode for a host that owns several cells: one TTI of up to n_cells cells in one kernel launch, one workgroup per cell
    (rs_group_create / rs_group_schedule_tti).  Cell k behaves exactly like a TtiScheduler of its own."""

    def __init__(self, slices: SliceConfig, n_rbgs: int, rbg_size: int, n_cells: int, sched: int = RS_SCHED_MAXCELL,
                 device: int = 0, stream: Optional[int] = None, synthetic_exp: bool = False, link_tables: int = RS_LINK_DEFAULT,
                 jit: bool = False, jit_resident: bool = False, jit_queued: bool = False, jit_counted: bool = False, jit_flows: bool = False,
                 jit_run: bool = False):
        """jit: specialize() right after the group is created.  jit_resident: specialize_resident() as well (independent of jit).
        jit_queued: specialize_queued() as well (independent of both).  jit_counted / jit_flows: specialize_counted() /
        specialize_flows() as well (independent of all others).  jit_run: specialize_run() as well (independent of all others: the
        builds that serve run_at)."""
        self.slices, self.R, self.rbg_size, self.sched, self.n_cells = slices, n_rbgs, rbg_size, sched, n_cells
        self._cfg = _CfgHolder(slices, n_rbgs, rbg_size, sched, device, stream, synthetic_exp, link_tables)
        self._h = lib().rs_group_create_checked(C.byref(self._cfg.c), n_cells, RS_ABI_VERSION, C.sizeof(_Config))
        if not self._h:
            raise RadioSaberError(-1, lib().rs_last_error().decode())
        if jit:
            self.specialize()
        if jit_resident:
            self.specialize_resident()
        if jit_queued:
            self.specialize_queued()
        if jit_counted:
            self.specialize_counted()
        if jit_flows:
            self.specialize_flows()
        if jit_run:
            self.specialize_run()

    def specialize(self):
        """rs_group_specialize: the group's own hiprtc builds of the one-TTI kernel (identical results; their first calls run beside
        the built-in kernel unless the builds carry the self-check mark: jit_status()).  Any time between two calls; again: a no-op."""
        _check(lib().rs_group_specialize(self._h))

    def jit_status(self):
        """(code, message) of rs_group_jit_status: 1 the group's builds serve, 0 not asked for, -1 build failed, -2 dropped by the self-check."""
        buf = C.create_string_buffer(768)
        rc = lib().rs_group_jit_status(self._h, buf, 768)
        return rc, buf.value.decode(errors="replace")

    def specialize_resident(self):
        """rs_group_specialize_resident: the group's own hiprtc builds of the RESIDENT kernel, for schedule_tti_at (identical results;
        their first calls run beside the built-in resident kernel and are compared on outputs and on state -- slice state, averages,
        pending bytes, last update -- unless the builds carry the self-check mark: resident_jit_status()).  Independent of
        specialize(); any time between two calls; again: a no-op."""
        _check(lib().rs_group_specialize_resident(self._h))

    def resident_jit_status(self):
        """(code, message) of rs_group_resident_jit_status, for the resident builds alone: 1 they serve the resident calls, 0 not asked
        for, -1 build failed, -2 dropped by the self-check."""
        buf = C.create_string_buffer(768)
        rc = lib().rs_group_resident_jit_status(self._h, buf, 768)
        return rc, buf.value.decode(errors="replace")

    def specialize_queued(self):
        """rs_group_specialize_queued: the group's own hiprtc builds of the QUEUED kernel, for schedule_tti_queued (identical results;
        their first calls run beside the built-in queued kernel and are compared on outputs and on state -- slice state, both bearers'
        averages and pending bytes of every user, last update -- unless the builds carry the self-check mark: queued_jit_status()).
        Independent of specialize() and specialize_resident(); any time between two calls; again: a no-op."""
        _check(lib().rs_group_specialize_queued(self._h))

    def queued_jit_status(self):
        """(code, message) of rs_group_queued_jit_status, for the queued builds alone: 1 they serve the queued calls, 0 not asked for,
        -1 build failed, -2 dropped by the self-check."""
        buf = C.create_string_buffer(768)
        rc = lib().rs_group_queued_jit_status(self._h, buf, 768)
        return rc, buf.value.decode(errors="replace")

    def specialize_counted(self):
        """rs_group_specialize_counted: the group's own hiprtc builds of the COUNTED kernel, for schedule_tti_counted (identical results;
        their first calls run beside the built-in counted kernel and are compared on outputs, sent rows and state -- slice state, both
        bearers' averages, pending bytes, cum_bytes and cum_rbs of every user, last update -- unless the builds carry the self-check
        mark: counted_jit_status()).  Independent of the other pairs; any time between two calls; again: a no-op."""
        _check(lib().rs_group_specialize_counted(self._h))

    def counted_jit_status(self):
        """(code, message) of rs_group_counted_jit_status, for the counted builds alone: 1 they serve the counted calls, 0 not asked
        for, -1 build failed, -2 dropped by the self-check."""
        buf = C.create_string_buffer(768)
        rc = lib().rs_group_counted_jit_status(self._h, buf, 768)
        return rc, buf.value.decode(errors="replace")

    def specialize_flows(self):
        """rs_group_specialize_flows: the group's own hiprtc builds of scheduler 1's FLOWS kernel, for schedule_tti_flows (identical
        results; their first calls run beside the built-in flows kernel and are compared on outputs and on state -- slice state, both
        bearers' averages, pending bytes, cum_bytes and cum_rbs of every user, last update -- unless the builds carry the self-check
        mark: flows_jit_status()).  Independent of the other pairs; any time between two calls; again: a no-op."""
        _check(lib().rs_group_specialize_flows(self._h))

    def flows_jit_status(self):
        """(code, message) of rs_group_flows_jit_status, for the flows builds alone: 1 they serve the flows calls, 0 not asked for,
        -1 build failed, -2 dropped by the self-check."""
        buf = C.create_string_buffer(768)
        rc = lib().rs_group_flows_jit_status(self._h, buf, 768)
        return rc, buf.value.decode(errors="replace")

    def specialize_run(self):
        """rs_group_specialize_run: the group's own hiprtc builds of the RUN kernel, for run_at (identical results; their first runs
        execute beside the built-in run kernel and are compared on the outputs of every (cell, TTI) and on state -- slice state,
        averages and pending bytes of every user id, last update -- unless the builds carry the self-check mark: run_jit_status()).
        Independent of the other five pairs -- specialize_resident() does not reach runs, this does not reach schedule_tti_at --; any
        time between two calls; again: a no-op."""
        _check(lib().rs_group_specialize_run(self._h))

    def run_jit_status(self):
        """(code, message) of rs_group_run_jit_status, for the run builds alone: 1 they serve the runs, 0 not asked for, -1 build
        failed, -2 dropped by the self-check."""
        buf = C.create_string_buffer(768)
        rc = lib().rs_group_run_jit_status(self._h, buf, 768)
        return rc, buf.value.decode(errors="replace")

    def close(self):
        if getattr(self, "_h", None):
            lib().rs_group_destroy(self._h)
            self._h = None

    __del__ = close

    def schedule_tti(self, calls: Sequence[dict], cell_ids: Optional[Sequence[int]] = None) -> List[TtiResult]:
        """calls[k]: the keyword arguments of TtiScheduler.schedule_tti for cell cell_ids[k] (None: cell k).  Optional inputs are
        given by every cell of a call or by none (a mixed call raises, nothing is launched).  cqi_epoch counts per cell: a cell whose
        call repeats the number, users and kind of report of its last stored call is served from its device-resident image."""
        n = len(calls)
        ins, outs, results, keep = (_TtiIn * n)(), (_TtiOut * n)(), [], []
        for k, kw in enumerate(calls):
            kw = dict(kw)
            tin, tout, res, arrays = _marshal_tti(self.slices.n_slices, self.R, self.rbg_size, self.sched, kw.pop("cqi", None),
                                                  kw.pop("avg_rate"), **kw)
            ins[k], outs[k] = tin, tout
            results.append(res)
            keep.append(arrays)
        ids = None if cell_ids is None else np.ascontiguousarray(cell_ids, np.int32)
        assert ids is None or ids.shape == (n,)
        _check(lib().rs_group_schedule_tti(self._h, n, _p(ids, C.c_int32) if ids is not None else None, ins, outs))
        return results

    # ---- resident averages: the cell's PF averages, pending bytes and last-update time stay on the device ----
    def set_avg(self, cell, avg, last_update):
        """rs_group_set_avg: makes `cell` resident with avg [n_users] by user id (1 <= avg <= 2**52), zero pending bytes and
        last_update (RadioBearer's m_lastUpdate).  Any time between two calls."""
        a = np.ascontiguousarray(avg, np.float64)
        assert a.shape == (self.slices.n_users,)
        _check(lib().rs_group_set_avg(self._h, cell, _p(a, C.c_double), float(last_update)))

    def get_avg(self, cell):
        """(avg float64 [n_users], pending bytes int32 [n_users], last_update) of a resident cell: a synchronising copy, not part of a TTI."""
        a = np.zeros(self.slices.n_users, np.float64)
        pend = np.zeros(self.slices.n_users, np.int32)
        last = C.c_double(0)
        _check(lib().rs_group_get_avg(self._h, cell, _p(a, C.c_double), _p(pend, C.c_int32), C.byref(last)))
        return a, pend, float(last.value)

    def set_pending(self, cell, pending_bytes):
        """rs_group_set_pending: overwrites the bytes that wait for the cell's next update (finite queues: what DoStopSchedule
        credited instead of the transport blocks).  Outside the fast path."""
        b = np.ascontiguousarray(pending_bytes, np.int32)
        assert b.shape == (self.slices.n_users,)
        _check(lib().rs_group_set_pending(self._h, cell, _p(b, C.c_int32)))

    def schedule_tti_at(self, calls: Sequence[dict], now, cell_ids: Optional[Sequence[int]] = None) -> List[TtiResult]:
        """rs_group_schedule_tti_at: schedule_tti for resident cells.  calls[k] as for schedule_tti but without avg_rate; now[k] is
        the simulator clock of that cell's TTI (a scalar: the same for every cell).  Per cell the device applies the reference's
        EWMA to every user's average, schedules the TTI on the result and records the grants for the next update."""
        n = len(calls)
        ins, outs, results, keep = (_TtiIn * n)(), (_TtiOut * n)(), [], []
        for k, kw in enumerate(calls):
            kw = dict(kw)
            tin, tout, res, arrays = _marshal_tti(self.slices.n_slices, self.R, self.rbg_size, self.sched, kw.pop("cqi", None),
                                                  kw.pop("avg_rate", None), **kw)
            ins[k], outs[k] = tin, tout
            results.append(res)
            keep.append(arrays)
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(now, np.float64), (n,)))
        ids = None if cell_ids is None else np.ascontiguousarray(cell_ids, np.int32)
        assert ids is None or ids.shape == (n,)
        _check(lib().rs_group_schedule_tti_at(self._h, n, _p(ids, C.c_int32) if ids is not None else None, ins, outs, _p(t, C.c_double)))
        return results

    def run_at(self, calls: Sequence[dict], now, rands=None, cell_ids: Optional[Sequence[int]] = None) -> List[List[TtiResult]]:
        """rs_group_run_at: T consecutive schedule_tti_at calls in one launch.  calls[k] as for schedule_tti_at, given once per cell
        (rand0 / rand1 are not read); now is [T] (the same clock for every cell) or [n][T]; rands is [n][T][2], the rand() pair of each
        cell's TTIs (None: RS_SCHED_PF only).  Returns results[k][t]."""
        return self._run(lib().rs_group_run_at, calls, now, rands, cell_ids, True)

    def _run(self, fn, calls, now, rands, cell_ids, outputs, rec=None):
        """rec: (rec_cap, recs, n_recs) -- the three extra arguments of rs_group_run_records_at (arrays, or None for a NULL pointer)"""
        n = len(calls)
        t = np.asarray(now, np.float64)
        assert t.ndim in (1, 2) and (t.ndim == 1 or t.shape[0] == n)
        T = t.shape[-1]
        t = np.ascontiguousarray(np.broadcast_to(t, (n, T)))
        r = None if rands is None else np.ascontiguousarray(rands, np.int32)
        assert r is None or r.shape == (n, T, 2)
        ins, outs, results, keep = (_TtiIn * n)(), (_TtiOut * (n * max(T, 1)))(), [], []
        for k, kw in enumerate(calls):
            kw = dict(kw)
            cqi, avg = kw.pop("cqi", None), kw.pop("avg_rate", None)
            row = []
            for j in range(max(T, 1)):  # (one rs_tti_out per TTI; the rs_tti_in is the first one's)
                tin, tout, res, arrays = _marshal_tti(self.slices.n_slices, self.R, self.rbg_size, self.sched, cqi, avg, **kw)
                if j == 0:
                    ins[k] = tin
                outs[k * max(T, 1) + j] = tout
                row.append(res)
                keep.append(arrays)
            results.append(row[:T])
        ids = None if cell_ids is None else np.ascontiguousarray(cell_ids, np.int32)
        assert ids is None or ids.shape == (n,)
        more = () if rec is None else (int(rec[0]), rec[1].ctypes.data if rec[1] is not None else None,
                                       _p(rec[2], C.c_int32) if rec[2] is not None else None)
        _check(fn(self._h, n, _p(ids, C.c_int32) if ids is not None else None, ins, T, _p(t, C.c_double),
                  _p(r, C.c_int32) if r is not None else None, outs if outputs else None, *more))
        return results if outputs else None

    # ---- counted runs: m_cumulateBytes / m_cumulateRBs per user of an average-resident cell stay on the device too ----
    def set_avg_counters(self, cell, cum_bytes=None, cum_rbs=None):
        """rs_group_set_avg_counters: makes an average-resident `cell` avg-counted with cum_bytes / cum_rbs int64 [n_users] by user id
        (None: zeros).  Any time between two calls; outside the fast path."""
        U = self.slices.n_users
        cb = None if cum_bytes is None else np.ascontiguousarray(cum_bytes, np.int64)
        cr = None if cum_rbs is None else np.ascontiguousarray(cum_rbs, np.int64)
        assert (cb is None or cb.shape == (U,)) and (cr is None or cr.shape == (U,))
        _check(lib().rs_group_set_avg_counters(self._h, cell, _p(cb, C.c_int64) if cb is not None else None,
                                               _p(cr, C.c_int64) if cr is not None else None))

    def get_avg_counters(self, cell):
        """(cum_bytes int64 [n_users], cum_rbs int64 [n_users]) of an avg-counted cell: a synchronising copy, not part of a TTI."""
        U = self.slices.n_users
        cb = np.zeros(U, np.int64)
        cr = np.zeros(U, np.int64)
        _check(lib().rs_group_get_avg_counters(self._h, cell, _p(cb, C.c_int64), _p(cr, C.c_int64)))
        return cb, cr

    def run_counted_at(self, calls: Sequence[dict], now, rands=None, cell_ids: Optional[Sequence[int]] = None, outputs=True,
                       records=False, rec_cap=None):
        """rs_group_run_counted_at: run_at for avg-counted cells, same calls and same results; every grant also adds its bytes and the
        position's PRBs to the user's counters.  outputs=False is the output-free run: nothing is written per TTI or unpacked, state
        and counters are what the run with outputs leaves, and the call returns None; else results[k][t].
        records=True is rs_group_run_records_at: the same run, and the call returns (results or None, recs) with recs[k][t] a
        GRANT_RECORD array of that cell's grants in that TTI, ascending in pos -- what logfmt.run_record_lines makes the reference's
        app: lines of.  rec_cap (default and least: grant_bound) is the room per TTI."""
        if not records:
            return self._run(lib().rs_group_run_counted_at, calls, now, rands, cell_ids, outputs)
        n, T = len(calls), np.asarray(now).shape[-1]
        cap = self.grant_bound if rec_cap is None else int(rec_cap)
        recs = np.zeros((n, T, max(cap, 1)), GRANT_RECORD)
        n_recs = np.zeros((n, T), np.int32)
        res = self._run(lib().rs_group_run_records_at, calls, now, rands, cell_ids, outputs, rec=(cap, recs, n_recs))
        return res, [[recs[k, t, :n_recs[k, t]].copy() for t in range(T)] for k in range(n)]

    @property
    def grant_bound(self):
        """rs_group_grant_bound: the most grants one cell can have in one TTI -- the least rec_cap of a run with records."""
        return _count(lib().rs_group_grant_bound(self._h))

    # ---- resident bearers: both bearers of every user stay on the device, finite queues are credited there ----
    def set_bearers(self, cell, has_bearer, avg, last_update):
        """rs_group_set_bearers: makes `cell` bearer-resident with has_bearer [n_users][2] and avg [n_users][2] by user id and bearer
        priority (1 <= avg <= 2**51 where the bearer exists), zero pending bytes and last_update.  Any time between two calls."""
        U = self.slices.n_users
        h = np.ascontiguousarray(has_bearer, np.uint8)
        a = np.ascontiguousarray(avg, np.float64)
        assert h.shape == (U, 2) and a.shape == (U, 2)
        _check(lib().rs_group_set_bearers(self._h, cell, _p(h, C.c_uint8), _p(a, C.c_double), float(last_update)))

    def get_bearers(self, cell):
        """(avg float64 [n_users][2], pending bytes int32 [n_users][2], last_update) of a bearer-resident cell, 0 for a bearer that does
        not exist: a synchronising copy, not part of a TTI."""
        U = self.slices.n_users
        a = np.zeros((U, 2), np.float64)
        pend = np.zeros((U, 2), np.int32)
        last = C.c_double(0)
        _check(lib().rs_group_get_bearers(self._h, cell, _p(a, C.c_double), _p(pend, C.c_int32), C.byref(last)))
        return a, pend, float(last.value)

    def schedule_tti_queued(self, calls: Sequence[dict], now, cell_ids: Optional[Sequence[int]] = None) -> List[TtiResult]:
        """rs_group_schedule_tti_queued: schedule_tti for bearer-resident cells.  calls[k] as for schedule_tti_at plus data_to_transmit
        [n][2], UserToSchedule::m_dataToTransmit of the call's users by bearer priority; or dict(n_users=0), an update-only slot:
        the cell's bearers get their EWMA step at now[k] and nothing is scheduled (its result reads rbg_to_user -1, targets and quotas 0)."""
        return self._schedule_queued(calls, now, cell_ids, False)

    def _schedule_queued(self, calls, now, cell_ids, counted):
        n = len(calls)
        S, R = self.slices.n_slices, self.R
        ins, outs, results, keep = (_TtiIn * n)(), (_TtiOut * n)(), [], []
        data = (C.POINTER(C.c_int32) * n)()
        sent = (C.POINTER(C.c_int32) * n)()
        for k, kw in enumerate(calls):
            kw = dict(kw)
            if kw.get("n_users", None) == 0:
                assert len(kw) == 1, "an update-only slot gives nothing but n_users=0"
                z = np.zeros(0, np.int32)
                res = TtiResult(np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(R, np.int32), z, z.copy(), z.copy(), z.copy())
                ins[k] = _TtiIn()
                outs[k] = _TtiOut(_p(res.target_rbs, C.c_int32), _p(res.quota_rbgs, C.c_int32), _p(res.rbg_to_user, C.c_int32),
                                  None, None, None, None, None, None)
                if counted:
                    res.sent = np.zeros((0, 2), np.int32)
                results.append(res)
                continue
            d = np.ascontiguousarray(kw.pop("data_to_transmit"), np.int32)
            tin, tout, res, arrays = _marshal_tti(S, R, self.rbg_size, self.sched, kw.pop("cqi", None), kw.pop("avg_rate", None), **kw)
            assert d.shape == (tin.n_users, 2)
            ins[k], outs[k] = tin, tout
            data[k] = _p(d, C.c_int32)
            if counted:
                res.sent = np.zeros((tin.n_users, 2), np.int32)
                sent[k] = _p(res.sent, C.c_int32)
            results.append(res)
            keep.append((arrays, d))
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(now, np.float64), (n,)))
        ids = None if cell_ids is None else np.ascontiguousarray(cell_ids, np.int32)
        assert ids is None or ids.shape == (n,)
        idp = _p(ids, C.c_int32) if ids is not None else None
        if counted:
            _check(lib().rs_group_schedule_tti_counted(self._h, n, idp, ins, outs, _p(t, C.c_double), data, sent))
        else:
            _check(lib().rs_group_schedule_tti_queued(self._h, n, idp, ins, outs, _p(t, C.c_double), data))
        return results

    # ---- counted bearers: m_cumulateBytes / m_cumulateRBs of a bearer-resident cell stay on the device too ----
    def set_counters(self, cell, cum_bytes=None, cum_rbs=None):
        """rs_group_set_counters: makes a bearer-resident `cell` counted with cum_bytes / cum_rbs int64 [n_users][2] by user id and
        bearer priority (None: zeros).  Any time between two calls; outside the fast path."""
        U = self.slices.n_users
        cb = None if cum_bytes is None else np.ascontiguousarray(cum_bytes, np.int64)
        cr = None if cum_rbs is None else np.ascontiguousarray(cum_rbs, np.int64)
        assert (cb is None or cb.shape == (U, 2)) and (cr is None or cr.shape == (U, 2))
        _check(lib().rs_group_set_counters(self._h, cell, _p(cb, C.c_int64) if cb is not None else None,
                                           _p(cr, C.c_int64) if cr is not None else None))

    def get_counters(self, cell):
        """(cum_bytes int64 [n_users][2], cum_rbs int64 [n_users][2]) of a counted cell: a synchronising copy, not part of a TTI."""
        U = self.slices.n_users
        cb = np.zeros((U, 2), np.int64)
        cr = np.zeros((U, 2), np.int64)
        _check(lib().rs_group_get_counters(self._h, cell, _p(cb, C.c_int64), _p(cr, C.c_int64)))
        return cb, cr

    def schedule_tti_counted(self, calls: Sequence[dict], now, cell_ids: Optional[Sequence[int]] = None) -> List[TtiResult]:
        """rs_group_schedule_tti_counted: schedule_tti_queued for counted cells, same calls and same results; each bearer credited also
        adds the bytes and the position's PRBs to its counters, and every TtiResult carries .sent [n][2], the bytes sent per call
        position and bearer (what a binding hands to UpdateTransmittedBytes and the RLC); an update-only slot gives an empty array."""
        return self._schedule_queued(calls, now, cell_ids, True)

    # ---- resident flows (scheduler 1): a call position is one bearer of one user, the whole block is credited to it ----
    def set_flows(self, cell, has_bearer, avg, last_update, cum_bytes=None, cum_rbs=None):
        """rs_group_set_flows: makes `cell` of a scheduler-1 group flow-resident with has_bearer [n_users][2] and avg [n_users][2] by
        user id and bearer index (1 <= avg <= 2**51 where the bearer exists), zero pending bytes, last_update and the counters
        cum_bytes / cum_rbs int64 [n_users][2] (None: zeros).  Any time between two calls."""
        U = self.slices.n_users
        h = np.ascontiguousarray(has_bearer, np.uint8)
        a = np.ascontiguousarray(avg, np.float64)
        cb = None if cum_bytes is None else np.ascontiguousarray(cum_bytes, np.int64)
        cr = None if cum_rbs is None else np.ascontiguousarray(cum_rbs, np.int64)
        assert h.shape == (U, 2) and a.shape == (U, 2) and (cb is None or cb.shape == (U, 2)) and (cr is None or cr.shape == (U, 2))
        _check(lib().rs_group_set_flows(self._h, cell, _p(h, C.c_uint8), _p(a, C.c_double), float(last_update),
                                        _p(cb, C.c_int64) if cb is not None else None, _p(cr, C.c_int64) if cr is not None else None))

    def get_flows(self, cell):
        """(avg float64, pending bytes int32, last_update, cum_bytes int64, cum_rbs int64) of a flow-resident cell, the arrays
        [n_users][2] and 0 for a bearer that does not exist: a synchronising copy, not part of a TTI."""
        U = self.slices.n_users
        a, pend = np.zeros((U, 2), np.float64), np.zeros((U, 2), np.int32)
        cb, cr = np.zeros((U, 2), np.int64), np.zeros((U, 2), np.int64)
        last = C.c_double(0)
        _check(lib().rs_group_get_flows(self._h, cell, _p(a, C.c_double), _p(pend, C.c_int32), C.byref(last), _p(cb, C.c_int64),
                                        _p(cr, C.c_int64)))
        return a, pend, float(last.value), cb, cr

    def schedule_tti_flows(self, calls: Sequence[dict], now, cell_ids: Optional[Sequence[int]] = None) -> List[TtiResult]:
        """rs_group_schedule_tti_flows: one TTI of flow-resident cells.  calls[k]: dict(user_id [n], flow_bearer [n] (0 or 1),
        data_to_transmit [n] (> 0), cqi [n][R] or cqi_prb [n][R * rbg_size], cqi_epoch) -- position i is bearer flow_bearer[i] of user
        user_id[i] (None: user i), the pairs ascending; or dict(n_users=0), an update-only slot.  Results are per position, and
        rbg_to_user holds flow ids 2 * user + bearer; the bytes credited to position i are user_tbs_bits[i] // 8."""
        n = len(calls)
        S, R = self.slices.n_slices, self.R
        ins, outs, results, keep = (_TtiIn * n)(), (_TtiOut * n)(), [], []
        bearer = (C.POINTER(C.c_uint8) * n)()
        for k, kw in enumerate(calls):
            kw = dict(kw)
            if kw.get("n_users", None) == 0:
                assert len(kw) == 1, "an update-only slot gives nothing but n_users=0"
                z = np.zeros(0, np.int32)
                res = TtiResult(np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(R, np.int32), z, z.copy(), z.copy(), z.copy())
                ins[k] = _TtiIn()
                outs[k] = _TtiOut(_p(res.target_rbs, C.c_int32), _p(res.quota_rbgs, C.c_int32), _p(res.rbg_to_user, C.c_int32),
                                  None, None, None, None, None, None)
                results.append(res)
                continue
            fb = np.ascontiguousarray(kw.pop("flow_bearer"), np.uint8)
            tin, tout, res, arrays = _marshal_tti(S, R, self.rbg_size, self.sched, kw.pop("cqi", None), kw.pop("avg_rate", None), **kw)
            assert fb.shape == (tin.n_users,)
            ins[k], outs[k] = tin, tout
            bearer[k] = _p(fb, C.c_uint8)
            results.append(res)
            keep.append((arrays, fb))
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(now, np.float64), (n,)))
        ids = None if cell_ids is None else np.ascontiguousarray(cell_ids, np.int32)
        assert ids is None or ids.shape == (n,)
        _check(lib().rs_group_schedule_tti_flows(self._h, n, _p(ids, C.c_int32) if ids is not None else None, ins, outs, _p(t, C.c_double),
                                                 bearer))
        return results

    def slice_offset(self, cell):
        out = np.zeros(self.slices.n_slices, np.float64)
        _check(lib().rs_group_get_slice_offset(self._h, cell, _p(out, C.c_double)))
        return out

    def set_slice_offset(self, cell, v):
        a = np.ascontiguousarray(v, np.float64)
        assert a.shape == (self.slices.n_slices,)
        _check(lib().rs_group_set_slice_offset(self._h, cell, _p(a, C.c_double)))

    @property
    def launch_count(self):
        """scheduling kernels launched so far: one per successful schedule_tti"""
        return int(lib().rs_group_launch_count(self._h))

    @property
    def image_stats(self):
        """(cell-TTIs served from the cell's device-resident CQI image, cell-TTIs that stored one, cell-TTIs without a cqi_epoch) of
        the successful calls so far (rs_group_image_stats)"""
        out = np.zeros(3, np.int64)
        _check(lib().rs_group_image_stats(self._h, _p(out, C.c_int64)))
        return tuple(int(x) for x in out)

    @property
    def kernel_name(self):
        return lib().rs_group_kernel_name(self._h).decode()


class BatchScheduler:
    """Many independent cells resident on one MI355X (rs_batch_*)."""

    def __init__(self, slices: SliceConfig, n_rbgs: int, rbg_size: int, n_cells: int,
                 sched: int = RS_SCHED_MAXCELL, device: int = 0, first_tti: int = 100, cqi_refresh: int = 40,
                 phy_error_draws: bool = False, threads_per_cell: int = 0, stream: Optional[int] = None,
                 jit: bool = False, synthetic_exp: bool = False, cqi_epoch_wrap: bool = False, queue_state_lds: int = 0,
                 autotune: bool = False, selfcheck=0, link_tables: int = RS_LINK_DEFAULT):
        """selfcheck: 0 / False = run-time builds without the self-check mark are checked against the built-in kernels before they serve
        (the default since ABI 11), 1 / True = every build, -1 = never.  link_tables: RS_LINK_* (default for batches: pinned glibc 2.35).
        synthetic_exp: the reference built with FIRST/SECOND_SYNTHETIC_EXP (transport blocks PRB by PRB; rs_config.synthetic_exp).
        cqi_epoch_wrap: the uploaded / synthesized epochs cycle instead of ending the run.  queue_state_lds: 0 auto, 1 LDS, -1 HBM."""
        self.slices, self.R, self.rbg_size, self.sched, self.n_cells = slices, n_rbgs, rbg_size, sched, n_cells
        self.S, self.U = slices.n_slices, slices.n_users
        self._cfg = _CfgHolder(slices, n_rbgs, rbg_size, sched, device, stream, synthetic_exp, link_tables)
        bc = _BatchConfig(self._cfg.c, n_cells, first_tti, cqi_refresh, int(phy_error_draws), threads_per_cell,
                          int(jit), int(bool(cqi_epoch_wrap)), int(queue_state_lds), int(bool(autotune)), int(selfcheck))
        self._h = lib().rs_batch_create_checked(C.byref(bc), RS_ABI_VERSION, C.sizeof(_BatchConfig))
        if not self._h:
            raise RadioSaberError(-1, lib().rs_last_error().decode())

    def close(self):
        if getattr(self, "_h", None):
            lib().rs_batch_destroy(self._h)
            self._h = None

    __del__ = close

    def seed(self, seeds, rand_skip=None):
        s = np.ascontiguousarray(seeds, np.uint32)
        assert s.shape == (self.n_cells,)
        k = None if rand_skip is None else np.ascontiguousarray(rand_skip, np.int64)
        _check(lib().rs_batch_seed(self._h, _p(s, C.c_uint32), _p(k, C.c_int64) if k is not None else None))

    def upload_cqi_epochs(self, cqi):
        a = np.ascontiguousarray(cqi, np.uint8)
        assert a.ndim == 4 and a.shape[0] == self.n_cells and a.shape[2:] == (self.U, self.R), a.shape
        _check(lib().rs_batch_upload_cqi_epochs(self._h, _p(a, C.c_uint8), a.shape[1]))
        self.n_epochs = a.shape[1]

    def upload_cqi_epochs_prb(self, cqi_prb):
        """[n_cells][n_epochs][U][R*rbg_size]: per-PRB reports (the metric reads each RBG's first PRB, link adaptation all)."""
        a = np.ascontiguousarray(cqi_prb, np.uint8)
        assert a.ndim == 4 and a.shape[0] == self.n_cells and a.shape[2:] == (self.U, self.R * self.rbg_size), a.shape
        _check(lib().rs_batch_upload_cqi_epochs_prb(self._h, _p(a, C.c_uint8), a.shape[1]))
        self.n_epochs = a.shape[1]

    def set_trace_prb(self, trace_prb, user_trace, row_modulus=475):
        t = np.ascontiguousarray(trace_prb, np.uint8)
        assert t.ndim == 3 and t.shape[2] == self.R * self.rbg_size
        ut = np.ascontiguousarray(user_trace, np.int32)
        assert ut.shape == (self.n_cells, self.U)
        _check(lib().rs_batch_set_trace_prb(self._h, _p(t, C.c_uint8), t.shape[0], t.shape[1], row_modulus, _p(ut, C.c_int32)))

    def synthesize_cqi(self, seed, n_epochs, weights=TRACE_CQI_HISTOGRAM, first_cell=0):
        """Grids drawn on the device, keyed by (seed, first_cell + local cell, epoch, user, rbg)."""
        w = np.ascontiguousarray(weights, np.float64)
        assert w.shape == (15,)
        _check(lib().rs_batch_synthesize_cqi_at(self._h, seed, _p(w, C.c_double), n_epochs, first_cell))
        self.n_epochs = n_epochs

    def download_cqi_epochs(self, cell):
        out = np.zeros((self.n_epochs, self.U, self.R), np.uint8)
        _check(lib().rs_batch_download_cqi_epochs(self._h, cell, _p(out, C.c_uint8)))
        return out

    def set_trace(self, trace, user_trace, row_modulus=475):
        t = np.ascontiguousarray(trace, np.uint8)
        assert t.ndim == 3 and t.shape[2] == self.R
        ut = np.ascontiguousarray(user_trace, np.int32)
        assert ut.shape == (self.n_cells, self.U)
        _check(lib().rs_batch_set_trace(self._h, _p(t, C.c_uint8), t.shape[0], t.shape[1], row_modulus,
                                        _p(ut, C.c_int32)))

    def run(self, n_ttis):
        _check(lib().rs_batch_run(self._h, n_ttis))

    def run_async(self, n_ttis):
        _check(lib().rs_batch_run_async(self._h, n_ttis))

    def sync(self):
        _check(lib().rs_batch_sync(self._h))

    def run_logged(self, n_ttis, slice_keys=False, bearers=False):
        """slice_keys=True (transport schedulers) adds what the inter-slice step read: 'slice_cqi' [cells][ttis][R][S]
        (CQI of the slice's best user, 0 = no user) and 'slice_user' (its id, -1 = none).  bearers=True (queue model) adds the
        DoStopSchedule rows of every bearer: 'bearer_bytes' int32 [cells][ttis][U][2] (bytes credited, 0 = no log line) and
        'bearer_hol' float64 [cells][ttis][U][2] (GetHeadOfLinePacketDelay before the RLC dequeue)."""
        m = np.zeros((self.n_cells, n_ttis, self.R), np.int16)
        tb = np.zeros((self.n_cells, n_ttis, self.U), np.int32)
        q = np.zeros((self.n_cells, n_ttis, self.S), np.int16)
        tg = np.zeros((self.n_cells, n_ttis, self.S), np.int16)
        ui = np.zeros((self.n_cells, n_ttis, self.U), np.int32)
        keys = np.zeros((self.n_cells, n_ttis, self.R, self.S), np.uint32) if slice_keys else None
        lg = _BatchLog(_p(m, C.c_int16), _p(tb, C.c_int32), _p(q, C.c_int16), _p(tg, C.c_int16), _p(ui, C.c_int32),
                       _p(keys, C.c_uint32) if slice_keys else None)
        if bearers:
            bb = np.zeros((self.n_cells, n_ttis, self.U, 2), np.int32)
            bh = np.zeros((self.n_cells, n_ttis, self.U, 2), np.float64)
            blg = _BatchBearerLog(_p(bb, C.c_int32), _p(bh, C.c_double))
            _check(lib().rs_batch_run_logged_bearers(self._h, n_ttis, C.byref(lg), C.byref(blg)))
        else:
            _check(lib().rs_batch_run_logged_ex(self._h, n_ttis, C.byref(lg)))
        out = {"rbg_to_user": m, "tbs_bits": tb, "quota": q, "target": tg, "nprb": ui & 0xFFFF,
               "final_cqi": (ui >> 16) & 0xFF, "mcs": (ui >> 24) & 0xFF}
        if slice_keys:
            out["slice_cqi"] = (keys & 0xFF).astype(np.int32)
            out["slice_user"] = (keys >> 8).astype(np.int32) - 1
        if bearers:
            out["bearer_bytes"], out["bearer_hol"] = bb, bh
        return out

    def record_bound(self):
        """rs_batch_record_bound: the most bearers DoStopSchedule can credit in one TTI of one cell (queue model)."""
        return _count(lib().rs_batch_record_bound(self._h))

    def run_records(self, n_ttis, cap=None):
        """run(n_ttis) that also returns, per cell, a BEARER_RECORD array with one record per bearer DoStopSchedule credited in these
        TTIs, in the order of the log's counter lines (rs_batch_run_records; what logfmt.BearerLogWriter.record_lines reads).  cap: the
        places per cell, default n_ttis * record_bound(), which cannot overflow.  A cell that counts more than cap raises
        RadioSaberError (RS_ERR_RANGE) after the launch has completed; the error carries .records (the lists as far as they were
        written) and .counts (the counts as counted)."""
        if cap is None:
            cap = max(int(n_ttis), 1) * self.record_bound()
        recs = np.zeros((self.n_cells, max(int(cap), 1)), BEARER_RECORD)
        n = np.zeros(self.n_cells, np.int64)
        rc = lib().rs_batch_run_records(self._h, n_ttis, cap, recs.ctypes.data_as(C.c_void_p), _p(n, C.c_int64))
        out = [recs[c, :min(int(n[c]), int(cap))] for c in range(self.n_cells)]  # (views: the block's untouched pages are never mapped)
        if rc == -5:
            err = RadioSaberError(rc, lib().rs_last_error().decode())
            err.records, err.counts = out, n
            raise err
        _check(rc)
        return out

    def run_timed(self, n_ttis, launches):
        ms = np.zeros(launches, np.float32)
        _check(lib().rs_batch_run_timed(self._h, n_ttis, launches, _p(ms, C.c_float)))
        return ms

    def state(self):
        avg = np.zeros((self.n_cells, self.U), np.float64)
        cb = np.zeros((self.n_cells, self.U), np.int64)
        cr = np.zeros((self.n_cells, self.U), np.int64)
        sl = np.zeros((self.n_cells, self.S), np.float64)
        _check(lib().rs_batch_read_state(self._h, _p(avg, C.c_double), _p(cb, C.c_int64), _p(cr, C.c_int64),
                                         _p(sl, C.c_double)))
        return {"avg_rate": avg, "cum_bytes": cb, "cum_rbs": cr, "slice_state": sl}

    def write_state(self, avg_rate=None, slice_state=None):
        """Set the PF averages [n_cells][U] (>= 1) and / or the slice state [n_cells][S] between launches (rs_batch_write_state)."""
        a = None if avg_rate is None else np.ascontiguousarray(avg_rate, np.float64)
        s = None if slice_state is None else np.ascontiguousarray(slice_state, np.float64)
        assert a is None or a.shape == (self.n_cells, self.U)
        assert s is None or s.shape == (self.n_cells, self.S)
        _check(lib().rs_batch_write_state(self._h, _p(a, C.c_double) if a is not None else None,
                                          _p(s, C.c_double) if s is not None else None))

    # ---- finite queues ----
    def set_bearers(self, bearer_kind):
        """bearer_kind [U][2] (index = bearer priority): BEARER_NONE / BEARER_BACKLOG / BEARER_QUEUE."""
        k = np.ascontiguousarray(bearer_kind, np.uint8)
        assert k.shape == (self.U, 2)
        _check(lib().rs_batch_set_bearers(self._h, _p(k, C.c_uint8)))
        self.bearer_kind = k

    def set_arrivals(self, bursts):
        """bursts[(cell, user, prio)] = (time f64[n], n_full i32[n], last_bytes i32[n]) for every finite-queue bearer that
        receives traffic (missing keys: no arrivals)."""
        nb = self.n_cells * self.U * 2
        off = np.zeros(nb + 1, np.int64)
        for (c, u, k), (t, _, _) in bursts.items():
            off[(c * self.U + u) * 2 + k + 1] = len(t)
        off = np.cumsum(off)
        total = int(off[-1])
        t_all = np.zeros(max(total, 1), np.float64)
        nf_all = np.zeros(max(total, 1), np.int32)
        la_all = np.zeros(max(total, 1), np.int32)
        for (c, u, k), (t, nf, la) in bursts.items():
            i = int(off[(c * self.U + u) * 2 + k])
            t_all[i:i + len(t)], nf_all[i:i + len(t)], la_all[i:i + len(t)] = t, nf, la
        _check(lib().rs_batch_set_arrivals(self._h, _p(off, C.c_int64), _p(t_all, C.c_double), _p(nf_all, C.c_int32),
                                           _p(la_all, C.c_int32)))
        self._burst_slots = {key: (int(off[(key[0] * self.U + key[1]) * 2 + key[2]]), len(v[0])) for key, v in bursts.items()}
        self._n_bursts = total

    def flow_record(self):
        """The flow completion record (rs_batch_flow_record), keyed like the `bursts` of set_arrivals:
        {(cell, user, prio): (done_tti int32[n], done_time f64[n])}, per burst the TTI (counted from the batch's first scheduled
        TTI) whose DoStopSchedule sent the burst's last packet and that TTI's clock value; -1 while the flow is not complete.
        The flow completion time is done_time - time."""
        if not hasattr(self, "_burst_slots"):
            raise RadioSaberError(-4, "flow_record() before set_arrivals()")
        tti = np.zeros(max(self._n_bursts, 1), np.int32)
        tm = np.zeros(max(self._n_bursts, 1), np.float64)
        _check(lib().rs_batch_flow_record(self._h, _p(tti, C.c_int32), _p(tm, C.c_double)))
        return {key: (tti[i:i + n].copy(), tm[i:i + n].copy()) for key, (i, n) in self._burst_slots.items()}

    def bearer_state(self):
        shp = (self.n_cells, self.U, 2)
        avg, cb, cr = np.zeros(shp, np.float64), np.zeros(shp, np.int64), np.zeros(shp, np.int64)
        qb, qp = np.zeros(shp, np.int32), np.zeros(shp, np.int32)
        _check(lib().rs_batch_read_bearer_state(self._h, _p(avg, C.c_double), _p(cb, C.c_int64), _p(cr, C.c_int64),
                                                _p(qb, C.c_int32), _p(qp, C.c_int32)))
        return {"avg_rate": avg, "cum_bytes": cb, "cum_rbs": cr, "queue_bytes": qb, "queue_packets": qp}

    def clock(self):
        """(t, last_update): the simulated time of the next TTI and RadioBearer::m_lastUpdate, per cell."""
        t = np.zeros(self.n_cells, np.float64)
        lu = np.zeros(self.n_cells, np.float64)
        _check(lib().rs_batch_read_clock(self._h, _p(t, C.c_double), _p(lu, C.c_double)))
        return t, lu

    def prepare_launch(self, n_ttis):
        """Build now the kernel an unlogged run(n_ttis) would build at its first launch (the lean build): keeps hiprtc out of timed runs."""
        _check(lib().rs_batch_prepare_launch(self._h, int(n_ttis)))

    def checkpoint(self):
        """Everything the batch carries from one launch to the next, as bytes (rs_batch_checkpoint_save)."""
        n = _count(lib().rs_batch_checkpoint_bytes(self._h))
        buf = C.create_string_buffer(n)
        _check(lib().rs_batch_checkpoint_save(self._h, buf, n))
        return buf.raw

    def restore(self, blob):
        """Continue from a checkpoint of a batch of the same shape (rs_batch_checkpoint_load); set the CQI source first."""
        _check(lib().rs_batch_checkpoint_load(self._h, blob, len(blob)))

    def debug_clocks(self):
        """(shader MHz [n_cells], ms [n_cells]) of the last launch, from the kernel's own two clocks (rs_batch_debug_clocks)."""
        mhz = np.zeros(self.n_cells, np.float64)
        ms = np.zeros(self.n_cells, np.float64)
        _check(lib().rs_batch_debug_clocks(self._h, _p(mhz, C.c_double), _p(ms, C.c_double)))
        return mhz, ms

    def autotune_report(self):
        """(candidates timed, text): what rs_batch_config.autotune measured and kept."""
        buf = C.create_string_buffer(1024)
        n = lib().rs_batch_autotune_report(self._h, buf, 1024)
        return n, buf.value.decode(errors="replace")

    def jit_status(self):
        """(code, message): 1 = shape-specialised kernel in use, 0 = not requested, -1 = requested but the build failed."""
        if not getattr(self, "_h", None):
            raise RadioSaberError(-4, "jit_status() of a closed batch")
        buf = C.create_string_buffer(512)
        rc = lib().rs_batch_jit_status(self._h, buf, 512)
        return rc, buf.value.decode(errors="replace")

    def slice_bytes(self):
        out = np.zeros(self.S, np.uint64)
        _check(lib().rs_batch_slice_bytes(self._h, _p(out, C.c_uint64)))
        return out

    def slice_bytes_into(self, device_ptr):
        """Reduce per-slice cumulative bytes into a device buffer (uint64[S]) on the batch's stream."""
        _check(lib().rs_batch_slice_bytes_device(self._h, C.c_void_p(device_ptr)))

    def heap_sorts(self):
        """int64[n_cells][3]: heap-sort fallbacks of the std::sort emulation so far, per cell and device site
        (0 workgroup level of the register form, 1 inside one wave's finish, 2 workgroup level of the LDS form)."""
        out = np.zeros((self.n_cells, 3), np.int64)
        _check(lib().rs_batch_debug_heap_sorts(self._h, _p(out, C.c_int64)))
        return out

    def debug_stamps(self, cell=0):
        out = np.zeros(20, np.uint64)
        _check(lib().rs_batch_debug_stamps(self._h, cell, _p(out, C.c_uint64)))
        return out

    @property
    def ttis_done(self):
        return lib().rs_batch_ttis_done(self._h)

    @property
    def stream(self):
        return lib().rs_batch_stream(self._h)

    @property
    def kernel_name(self):
        return lib().rs_batch_kernel_name(self._h).decode()
