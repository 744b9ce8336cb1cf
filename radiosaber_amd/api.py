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
from typing import List, NamedTuple, Optional, Sequence

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
RS_USER_ABSENT = -1  # user_to_slice of a cell's row in rs_batch_set_cell_configs: the users behind the cell's last one

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


class GroupForm(NamedTuple):
    """One form of a group call, as one row of rs_api.cpp's table of forms: its three C names follow from the key."""
    key: str              # "" for the plain form
    keywords: frozenset   # the keywords of jit_selfcheck / jit_cache_file / jit_cache_warm that select the form's builds
    flags: int            # ... and the rs_jit_cache_* flag bits of those builds

    @property
    def specialize(self):
        return "rs_group_specialize" + ("_" + self.key if self.key else "")

    @property
    def jit_status(self):
        return "rs_group_" + (self.key + "_" if self.key else "") + "jit_status"

    @property
    def selfcheck(self):
        return "rs_jit_selfcheck_group" + ("_" + self.key if self.key else "")


# the forms in the order of RS_GROUP_PLAIN .. RS_GROUP_RUN.  counted=True implies queued=True (the counted form is the queued
# form's twin: flag value 64 is valid only together with 32), so `counted` alone and `queued` with `counted` are the same row
GROUP_FORMS = tuple(GroupForm(key, frozenset(kws.split()), flags) for key, kws, flags in (
    ("", "group", 8),
    ("resident", "group resident", 24),
    ("queued", "group queued", 40),
    ("counted", "group queued counted", 104),
    ("flows", "group flows", 136),
    ("run", "group resident run", 280),
))
_FORM = {f.key: f for f in GROUP_FORMS}

_int, _i32, _i64, _f64, _u8, _size, _str, _ptr = C.c_int, C.c_int32, C.c_int64, C.c_double, C.c_uint8, C.c_size_t, C.c_char_p, C.c_void_p
_P = C.POINTER
_SHAPE = [_int] * 6                      # n_slices, n_users, n_rbgs, rbg_size, threads, sched
_MSG = [_str, _size]                     # a message buffer and its length
_SLOTS = [_ptr, _i32, _P(_i32), _P(_TtiIn)]               # a group, n, cell_ids, in[n]
_RUN = _SLOTS + [_i32, _P(_f64), _P(_i32), _P(_TtiOut)]   # ... n_ttis, now, rands, out
_CELL = [_ptr, _i32]                     # a group and one of its cells


def _form_prototypes(key):
    f = _FORM[key]
    return {f.specialize: (_int, [_ptr]), f.jit_status: (_int, [_ptr] + _MSG), f.selfcheck: (_int, _SHAPE + _MSG)}


# name -> (restype, argtypes) of every function include/radiosaber_hip.h declares, in the header's order (tests check that the
# header declares these and no others, and that the library exports them all)
PROTOTYPES = {
    "rs_last_error": (_str, []),
    "rs_abi_version": (_int, []),
    "rs_device_count": (_int, []),
    "rs_link_tables": (_int, [_P(_f64)] * 4),
    "rs_link_tables_pinned": (_int, [_P(_f64)] * 4),
    "rs_link_tables_compare": (_int, _MSG),
    "rs_get_rbg_size": (_int, [_int]),
    "rs_dl_prbs_for_bandwidth": (_int, [_f64]),
    "rs_create": (_ptr, [_P(_Config)]),
    "rs_create_checked": (_ptr, [_P(_Config), _int, _size]),
    "rs_destroy": (_int, [_ptr]),
    "rs_schedule_tti": (_int, [_ptr, _P(_TtiIn), _P(_TtiOut)]),
    "rs_ctx_specialize": (_int, [_ptr]),
    "rs_ctx_jit_status": (_int, [_ptr] + _MSG),
    "rs_jit_selfcheck_dropin": (_int, _SHAPE + _MSG),
    "rs_get_slice_offset": (_int, [_ptr, _P(_f64)]),
    "rs_set_slice_offset": (_int, [_ptr, _P(_f64)]),
    "rs_group_create": (_ptr, [_P(_Config), _i32]),
    "rs_group_create_checked": (_ptr, [_P(_Config), _i32, _int, _size]),
    "rs_group_destroy": (_int, [_ptr]),
    "rs_group_schedule_tti": (_int, _SLOTS + [_P(_TtiOut)]),
    "rs_group_get_slice_offset": (_int, _CELL + [_P(_f64)]),
    "rs_group_set_slice_offset": (_int, _CELL + [_P(_f64)]),
    "rs_group_launch_count": (_i64, [_ptr]),
    "rs_group_image_stats": (_int, [_ptr, _P(_i64)]),
    "rs_group_kernel_name": (_str, [_ptr]),
    **_form_prototypes(""),
    "rs_group_set_avg": (_int, _CELL + [_P(_f64), _f64]),
    "rs_group_get_avg": (_int, _CELL + [_P(_f64), _P(_i32), _P(_f64)]),
    "rs_group_set_pending": (_int, _CELL + [_P(_i32)]),
    "rs_group_schedule_tti_at": (_int, _SLOTS + [_P(_TtiOut), _P(_f64)]),
    **_form_prototypes("resident"),
    "rs_group_run_at": (_int, _RUN),
    **_form_prototypes("run"),
    "rs_group_set_avg_counters": (_int, _CELL + [_P(_i64), _P(_i64)]),
    "rs_group_get_avg_counters": (_int, _CELL + [_P(_i64), _P(_i64)]),
    "rs_group_run_counted_at": (_int, _RUN),
    "rs_group_grant_bound": (_int, [_ptr]),
    "rs_group_run_records_at": (_int, _RUN + [_i32, _ptr, _P(_i32)]),
    "rs_group_set_bearers": (_int, _CELL + [_P(_u8), _P(_f64), _f64]),
    "rs_group_get_bearers": (_int, _CELL + [_P(_f64), _P(_i32), _P(_f64)]),
    "rs_group_schedule_tti_queued": (_int, _SLOTS + [_P(_TtiOut), _P(_f64), _P(_P(_i32))]),
    **_form_prototypes("queued"),
    "rs_group_set_counters": (_int, _CELL + [_P(_i64), _P(_i64)]),
    "rs_group_get_counters": (_int, _CELL + [_P(_i64), _P(_i64)]),
    "rs_group_schedule_tti_counted": (_int, _SLOTS + [_P(_TtiOut), _P(_f64), _P(_P(_i32)), _P(_P(_i32))]),
    **_form_prototypes("counted"),
    "rs_group_set_flows": (_int, _CELL + [_P(_u8), _P(_f64), _f64, _P(_i64), _P(_i64)]),
    "rs_group_get_flows": (_int, _CELL + [_P(_f64), _P(_i32), _P(_f64), _P(_i64), _P(_i64)]),
    "rs_group_schedule_tti_flows": (_int, _SLOTS + [_P(_TtiOut), _P(_f64), _P(_P(_u8))]),
    **_form_prototypes("flows"),
    "rs_batch_create": (_ptr, [_P(_BatchConfig)]),
    "rs_batch_create_checked": (_ptr, [_P(_BatchConfig), _int, _size]),
    "rs_batch_destroy": (_int, [_ptr]),
    "rs_batch_seed": (_int, [_ptr, _P(C.c_uint32), _P(_i64)]),
    "rs_batch_set_cell_configs": (_int, [_ptr, _P(_f64), _P(_i32), _P(_i32), _P(_i32)]),
    "rs_batch_get_cell_config": (_int, [_ptr, _i32, _P(_f64), _P(_i32), _P(_i32), _P(_i32)]),
    "rs_batch_slice_totals": (_int, [_ptr, _P(_i64), _P(_i64)]),
    "rs_batch_cell_users": (_int, [_ptr, _P(_i32)]),
    "rs_batch_set_cell_configs_n": (_int, [_ptr, _P(_i32), _P(_f64), _P(_i32), _P(_i32), _P(_i32)]),
    "rs_batch_cell_slices": (_int, [_ptr, _P(_i32)]),
    "rs_batch_upload_cqi_epochs": (_int, [_ptr, _P(_u8), _i32]),
    "rs_batch_upload_cqi_epochs_prb": (_int, [_ptr, _P(_u8), _i32]),
    "rs_batch_synthesize_cqi": (_int, [_ptr, C.c_uint64, _P(_f64), _i32]),
    "rs_batch_synthesize_cqi_at": (_int, [_ptr, C.c_uint64, _P(_f64), _i32, _i64]),
    "rs_batch_download_cqi_epochs": (_int, [_ptr, _i32, _P(_u8)]),
    "rs_batch_set_cqi_epochs_device": (_int, [_ptr, _ptr, _size, _i32]),
    "rs_batch_write_cqi_epochs_device": (_int, [_ptr, _i32, _i32, _ptr, _size, C.c_uint32]),
    "rs_batch_cqi_write_status": (_int, [_ptr, _P(_i64), _P(_i32)]),
    "rs_batch_debug_cqi_image": (_int, [_ptr, _i32, _i32, _P(_u8), _size]),
    "rs_batch_set_trace": (_int, [_ptr, _P(_u8), _i32, _i32, _i32, _P(_i32)]),
    "rs_batch_set_trace_prb": (_int, [_ptr, _P(_u8), _i32, _i32, _i32, _P(_i32)]),
    "rs_lds_bytes_per_cell": (_int, [_int] * 5),
    "rs_hbm_copy_probe": (_int, [_int, C.c_uint64, _int, _P(_f64)]),
    "rs_trace_read_mapping": (_int, [_str, _P(_i32), _i32]),
    "rs_trace_read_ue_log": (_int, [_str, _i32, _i32, _i32, _P(_u8), _P(_u8)]),
    "rs_trace_load_dir": (_int, [_str, _i32, _i32, _i32, _i32, _P(_u8)]),
    "rs_batch_set_bearers": (_int, [_ptr, _P(_u8)]),
    "rs_batch_set_arrivals": (_int, [_ptr, _P(_i64), _P(_f64), _P(_i32), _P(_i32)]),
    "rs_batch_read_bearer_state": (_int, [_ptr, _P(_f64), _P(_i64), _P(_i64), _P(_i32), _P(_i32)]),
    "rs_internet_flow_arrivals": (_int, [_f64, _f64, _f64, C.c_uint32, _i32, _P(_f64), _P(_i32), _P(_i32)]),
    "rs_batch_flow_record": (_int, [_ptr, _P(_i32), _P(_f64)]),
    "rs_batch_run": (_int, [_ptr, _i32]),
    "rs_batch_run_async": (_int, [_ptr, _i32]),
    "rs_batch_sync": (_int, [_ptr]),
    "rs_batch_run_logged": (_int, [_ptr, _i32, _P(C.c_int16), _P(_i32), _P(C.c_int16), _P(C.c_int16), _P(_i32)]),
    "rs_batch_run_logged_ex": (_int, [_ptr, _i32, _P(_BatchLog)]),
    "rs_batch_run_logged_bearers": (_int, [_ptr, _i32, _P(_BatchLog), _P(_BatchBearerLog)]),
    "rs_batch_record_bound": (_int, [_ptr]),
    "rs_batch_run_records": (_int, [_ptr, _i32, _i64, _ptr, _P(_i64)]),
    "rs_batch_grant_bound": (_int, [_ptr]),
    "rs_batch_run_grant_records": (_int, [_ptr, _i32, _i64, _ptr, _P(_i64)]),
    "rs_batch_run_timed": (_int, [_ptr, _i32, _i32, _P(C.c_float)]),
    "rs_batch_read_state": (_int, [_ptr, _P(_f64), _P(_i64), _P(_i64), _P(_f64)]),
    "rs_batch_write_state": (_int, [_ptr, _P(_f64), _P(_f64)]),
    "rs_batch_checkpoint_bytes": (_i64, [_ptr]),
    "rs_batch_checkpoint_save": (_int, [_ptr, _ptr, _size]),
    "rs_batch_checkpoint_load": (_int, [_ptr, _ptr, _size]),
    "rs_batch_read_clock": (_int, [_ptr, _P(_f64), _P(_f64)]),
    "rs_batch_jit_status": (_int, [_ptr] + _MSG),
    "rs_batch_autotune_report": (_int, [_ptr] + _MSG),
    "rs_batch_prepare_launch": (_int, [_ptr, _i32]),
    "rs_batch_slice_bytes_device": (_int, [_ptr, _ptr]),
    "rs_batch_slice_bytes": (_int, [_ptr, _P(C.c_uint64)]),
    "rs_jit_selfcheck": (_int, _SHAPE + _MSG),
    "rs_jit_selfcheck_untuned": (_int, _SHAPE + _MSG),
    "rs_jit_selfcheck_queue": (_int, _SHAPE + _MSG),
    "rs_jit_selfcheck_grant_records": (_int, _SHAPE + [_int] + _MSG),
    "rs_jit_selfcheck_cell_configs": (_int, _SHAPE + [_int] + _MSG),
    "rs_jit_selfcheck_ragged_cells": (_int, _SHAPE + [_int] + _MSG),
    "rs_jit_selfcheck_ragged_slices": (_int, _SHAPE + [_int] + _MSG),
    "rs_jit_cache_stats": (None, [_P(C.c_longlong)]),
    "rs_jit_compiler_identity": (_str, []),
    "rs_jit_cache_file": (_int, _SHAPE + [_int] + _MSG),
    "rs_jit_cache_warm": (_int, _SHAPE + [_int] + _MSG),
    "rs_device_source_hash": (_str, []),
    "rs_batch_debug_heap_sorts": (_int, [_ptr, _P(_i64)]),
    "rs_ctx_debug_heap_sorts": (_int, [_ptr, _P(_i64)]),
    "rs_batch_debug_clocks": (_int, [_ptr, _P(_f64), _P(_f64)]),
    "rs_batch_debug_stamps": (_int, [_ptr, _i32, _P(C.c_uint64)]),
    "rs_batch_ttis_done": (_i64, [_ptr]),
    "rs_batch_stream": (_ptr, [_ptr]),
    "rs_batch_kernel_name": (_str, [_ptr]),
}
ABI_SYMBOLS = list(PROTOTYPES)
RS_CQI_WRITE_ASYNC = 1  # rs_batch_write_cqi_epochs_device: return after the enqueue

# rs_grant_record: one grant of one TTI of a counted run (32 bytes)
GRANT_RECORD = np.dtype([("pos", np.int32), ("user_id", np.int32), ("bytes", np.int32), ("nprb", np.int32),
                         ("cum_bytes", np.int64), ("cum_rbs", np.int64)])
assert GRANT_RECORD.itemsize == 32
# rs_bearer_record: one bearer that DoStopSchedule credited in one TTI of a queue-model batch (32 bytes)
BEARER_RECORD = np.dtype([("tti", np.int32), ("user", np.int32), ("bearer", np.int32), ("bytes", np.int32), ("nprb", np.int32),
                          ("reserved", np.int32), ("hol_delay", np.float64)])
assert BEARER_RECORD.itemsize == 32
# one grant of one TTI of a backlogged batch (rs_batch_grant_record, include/radiosaber_hip.h): what BatchScheduler.run_grant_records returns
BATCH_GRANT_RECORD = np.dtype([("tti", np.int32), ("user", np.int32), ("tbs_bits", np.int32), ("bytes", np.int32), ("rbg_mask", np.uint64),
                               ("nprb", np.int32), ("final_cqi", np.uint8), ("mcs", np.uint8), ("reserved", np.uint16)])
assert BATCH_GRANT_RECORD.itemsize == 32

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
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
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
    """a's data as a t* that keeps `a` alive; NULL for None.  The pointer to a's buffer costs a third of ndarray.ctypes.data_as, which
    builds a Python object per array; a read-only or empty array has no such buffer and takes that way."""
    if a is None:
        return None
    try:
        return C.POINTER(t)(t.from_buffer(a))
    except (TypeError, ValueError, BufferError):
        return a.ctypes.data_as(C.POINTER(t))


def _opt(x, dtype, shape=None):
    """An optional argument as a contiguous array of this dtype (and shape), or None: _p makes the NULL pointer of it.  (The refusals
    of the group calls are raised, not asserted: they hold under python -O too.)"""
    if x is None:
        return None
    a = np.ascontiguousarray(x, dtype)
    if shape is not None and a.shape != shape:
        raise AssertionError(f"an array of shape {a.shape} where {shape} is expected")
    return a


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
    form = _group_form(group, resident, queued, counted, flows, run)
    buf = C.create_string_buffer(4096)
    fn = lib().rs_jit_selfcheck_queue if queues else (lib().rs_jit_selfcheck_untuned if untuned else lib().rs_jit_selfcheck)
    if dropin:  # the drop-in entry point's one-TTI kernel of a context of this shape (rs_ctx_specialize)
        fn = lib().rs_jit_selfcheck_dropin
    if form:
        fn = getattr(lib(), form.selfcheck)
    n = fn(n_slices, n_users, n_rbgs, rbg_size, threads, sched, buf, 4096)
    if n < 0:
        raise RadioSaberError(n, buf.value.decode(errors="replace"))
    return n


def jit_selfcheck_grant_records(n_slices, n_users, n_rbgs, rbg_size, threads=512, sched=RS_SCHED_MAXCELL, lean=False):
    """Compile the records variant of the batch kernel of one shape (what run_grant_records builds at its first launch; hiprtc, no GPU
    needed): the general build, or with lean=True the lean one; returns the code size.  Scheduler 11 has none: RadioSaberError."""
    buf = C.create_string_buffer(4096)
    n = lib().rs_jit_selfcheck_grant_records(n_slices, n_users, n_rbgs, rbg_size, threads, sched, 1 if lean else 0, buf, 4096)
    if n < 0:
        raise RadioSaberError(n, buf.value.decode(errors="replace"))
    return n


def jit_selfcheck_cell_configs(n_slices, n_users, n_rbgs, rbg_size, threads=512, sched=RS_SCHED_MAXCELL, lean=False, ragged=False,
                               ragged_slices=False):
    """Compile the batch kernel of one shape with per-cell configuration rows (what set_cell_configs builds for a batch with jit=True;
    hiprtc, no GPU needed): the general build, or with lean=True the lean one; ragged=True: the build of a batch whose cells have
    different user counts (rows that end in RS_USER_ABSENT); ragged_slices=True: of a batch with a cell of fewer slices than n_slices
    (absent users included); returns the code size.  Scheduler 11 has none: RadioSaberError."""
    buf = C.create_string_buffer(4096)
    fn = lib().rs_jit_selfcheck_ragged_slices if ragged_slices else lib().rs_jit_selfcheck_ragged_cells if ragged else lib().rs_jit_selfcheck_cell_configs
    n = fn(n_slices, n_users, n_rbgs, rbg_size, threads, sched, 1 if lean else 0, buf, 4096)
    if n < 0:
        raise RadioSaberError(n, buf.value.decode(errors="replace"))
    return n


def jit_cache_stats():
    """This process's disk-cache counters of the run-time compiled kernels: dict(hits, misses, stores, rejected)."""
    out = (C.c_longlong * 4)()
    lib().rs_jit_cache_stats(out)
    return dict(zip(("hits", "misses", "stores", "rejected"), (int(x) for x in out)))


_FORM_KEYWORDS = ("run", "flows", "counted", "queued", "resident", "group")  # the most specific first: the one a refusal names


def _group_form(group, resident, queued=False, counted=False, flows=False, run=False):
    """The row of GROUP_FORMS that these keywords select (None when none is set: not a group's kernel); ValueError for a set that is
    no row, naming the first keyword that lacks what every form with it has, or meets one that no form with it has."""
    given = frozenset(k for k, v in zip(_FORM_KEYWORDS, (run, flows, counted, queued, resident, group)) if v)
    on = given | {"queued"} if counted else given
    if not on:
        return None
    for form in GROUP_FORMS:
        if form.keywords == on:
            return form

    def named(keywords):
        return " and ".join(f"{k}=True" for k in reversed(_FORM_KEYWORDS) if k in keywords)
    for k in _FORM_KEYWORDS:
        if k in on:
            rows = [form.keywords for form in GROUP_FORMS if k in form.keywords]
            needs, excludes = frozenset.intersection(*rows) - on, on - frozenset.union(*rows)
            if needs:
                raise ValueError(f"{k}=True needs {named(needs)}: a group's kernel has no form with {k}=True otherwise")
            if excludes:
                raise ValueError(f"{k}=True excludes {named(excludes & given)}: a group's kernel has no form with all of them")
    raise ValueError(f"{named(on)} select no form of a group's kernel")


def _jit_flags(lean, streamed, group, resident, queued=False, counted=False, flows=False, run=False):
    form = _group_form(group, resident, queued, counted, flows, run)
    return (4 if lean else 0) | (2 if streamed else 0) | (form.flags if form else 0)


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
                                           _p(prb, C.c_uint8)))
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
    avg = _opt(avg_rate, np.float64, (n,))  # (None: a resident call, GroupScheduler.schedule_tti_at)
    uid, hol, prio = _opt(user_id, np.int32), _opt(hol_delay, np.float64), _opt(prio_has_data, np.uint8)
    draws = _opt(rand_draws, np.int32)
    assert draws is None or draws.size == 300 * n
    req, dat = _opt(required_rbs, np.int32, (n,)), _opt(data_to_transmit, np.int32, (n,))
    res = TtiResult(np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(R, np.int32),
                    np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32))
    tin = _TtiIn(n, _p(uid, C.c_int32), _p(cqi, C.c_uint8), _p(avg, C.c_double), rand0, rand1, _p(prb, C.c_uint8), _p(hol, C.c_double),
                 _p(prio, C.c_uint8), _p(draws, C.c_int32), _p(req, C.c_int32), _p(dat, C.c_int32), int(cqi_epoch))
    if sched == RS_SCHED_UPPERBOUND:
        res.upper_rbg = np.full((S, R), -1, np.int32)
        res.upper_user = np.full((S, R), -1, np.int32)
    tout = _TtiOut(_p(res.target_rbs, C.c_int32), _p(res.quota_rbgs, C.c_int32),
                   _p(res.rbg_to_user, C.c_int32), _p(res.user_nprb, C.c_int32),
                   _p(res.user_final_cqi, C.c_int32), _p(res.user_mcs, C.c_int32),
                   _p(res.user_tbs_bits, C.c_int32), _p(res.upper_rbg, C.c_int32), _p(res.upper_user, C.c_int32))
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


class _GroupCall(NamedTuple):
    """One group call as GroupScheduler._marshal leaves it; whoever holds it keeps every array alive that the pointers name."""
    n: int
    ids: object      # int32* [n], or None
    ins: object      # rs_tti_in [n]
    outs: object     # rs_tti_out [n], of a run [n][max(T, 1)]
    now: object      # double* [n], of a run [n][T]; None for the call without a clock
    column: object   # the pointer column asked for, or None
    sent: object     # the pointer column to the results' sent rows, or None
    results: list
    keep: list


_NO_CLOCK = object()  # (not None: a clock of None is a NaN, as np.asarray reads it)


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
        for form, asked in zip(GROUP_FORMS, (jit, jit_resident, jit_queued, jit_counted, jit_flows, jit_run)):
            if asked:
                self._specialize(form.key)

    def _specialize(self, key):
        _check(getattr(lib(), _FORM[key].specialize)(self._h))

    def _jit_status(self, key):
        buf = C.create_string_buffer(768)
        rc = getattr(lib(), _FORM[key].jit_status)(self._h, buf, 768)
        return rc, buf.value.decode(errors="replace")

    def specialize(self):
        """rs_group_specialize: the group's own hiprtc builds of the one-TTI kernel (identical results; their first calls run beside
        the built-in kernel unless the builds carry the self-check mark: jit_status()).  Any time between two calls; again: a no-op."""
        self._specialize("")

    def jit_status(self):
        """(code, message) of rs_group_jit_status: 1 the group's builds serve, 0 not asked for, -1 build failed, -2 dropped by the self-check."""
        return self._jit_status("")

    def specialize_resident(self):
        """rs_group_specialize_resident: the group's own hiprtc builds of the RESIDENT kernel, for schedule_tti_at (identical results;
        their first calls run beside the built-in resident kernel and are compared on outputs and on state -- slice state, averages,
        pending bytes, last update -- unless the builds carry the self-check mark: resident_jit_status()).  Independent of
        specialize(); any time between two calls; again: a no-op."""
        self._specialize("resident")

    def resident_jit_status(self):
        """(code, message) of rs_group_resident_jit_status, for the resident builds alone: 1 they serve the resident calls, 0 not asked
        for, -1 build failed, -2 dropped by the self-check."""
        return self._jit_status("resident")

    def specialize_queued(self):
        """rs_group_specialize_queued: the group's own hiprtc builds of the QUEUED kernel, for schedule_tti_queued (identical results;
        their first calls run beside the built-in queued kernel and are compared on outputs and on state -- slice state, both bearers'
        averages and pending bytes of every user, last update -- unless the builds carry the self-check mark: queued_jit_status()).
        Independent of specialize() and specialize_resident(); any time between two calls; again: a no-op."""
        self._specialize("queued")

    def queued_jit_status(self):
        """(code, message) of rs_group_queued_jit_status, for the queued builds alone: 1 they serve the queued calls, 0 not asked for,
        -1 build failed, -2 dropped by the self-check."""
        return self._jit_status("queued")

    def specialize_counted(self):
        """rs_group_specialize_counted: the group's own hiprtc builds of the COUNTED kernel, for schedule_tti_counted (identical results;
        their first calls run beside the built-in counted kernel and are compared on outputs, sent rows and state -- slice state, both
        bearers' averages, pending bytes, cum_bytes and cum_rbs of every user, last update -- unless the builds carry the self-check
        mark: counted_jit_status()).  Independent of the other pairs; any time between two calls; again: a no-op."""
        self._specialize("counted")

    def counted_jit_status(self):
        """(code, message) of rs_group_counted_jit_status, for the counted builds alone: 1 they serve the counted calls, 0 not asked
        for, -1 build failed, -2 dropped by the self-check."""
        return self._jit_status("counted")

    def specialize_flows(self):
        """rs_group_specialize_flows: the group's own hiprtc builds of scheduler 1's FLOWS kernel, for schedule_tti_flows (identical
        results; their first calls run beside the built-in flows kernel and are compared on outputs and on state -- slice state, both
        bearers' averages, pending bytes, cum_bytes and cum_rbs of every user, last update -- unless the builds carry the self-check
        mark: flows_jit_status()).  Independent of the other pairs; any time between two calls; again: a no-op."""
        self._specialize("flows")

    def flows_jit_status(self):
        """(code, message) of rs_group_flows_jit_status, for the flows builds alone: 1 they serve the flows calls, 0 not asked for,
        -1 build failed, -2 dropped by the self-check."""
        return self._jit_status("flows")

    def specialize_run(self):
        """rs_group_specialize_run: the group's own hiprtc builds of the RUN kernel, for run_at (identical results; their first runs
        execute beside the built-in run kernel and are compared on the outputs of every (cell, TTI) and on state -- slice state,
        averages and pending bytes of every user id, last update -- unless the builds carry the self-check mark: run_jit_status()).
        Independent of the other five pairs -- specialize_resident() does not reach runs, this does not reach schedule_tti_at --; any
        time between two calls; again: a no-op."""
        self._specialize("run")

    def run_jit_status(self):
        """(code, message) of rs_group_run_jit_status, for the run builds alone: 1 they serve the runs, 0 not asked for, -1 build
        failed, -2 dropped by the self-check."""
        return self._jit_status("run")

    def close(self):
        if getattr(self, "_h", None):
            lib().rs_group_destroy(self._h)
            self._h = None

    __del__ = close

    _COLUMNS = {"data_to_transmit": (np.int32, C.c_int32, (2,)), "flow_bearer": (np.uint8, C.c_uint8, ())}  # dtype, C type, shape after [n]

    def _marshal(self, calls, cell_ids, now=_NO_CLOCK, T=None, need_avg=False, update_only=False, column=None, sent=False):
        """The arguments of one group call, as a _GroupCall.  now: broadcast to [n], or to [n][T] for a run of T TTIs, whose slots get
        max(T, 1) rs_tti_out each and a row of results.  need_avg: every slot gives avg_rate.  update_only: a slot may be
        dict(n_users=0).  column: the slot key that fills a pointer per slot ([n][2] int32 data_to_transmit, [n] uint8 flow_bearer)
        instead of going to _marshal_tti.  sent: every result gets its .sent [n][2], and the slots a pointer column to them."""
        n, m = len(calls), 1 if T is None else max(T, 1)
        S, R = self.slices.n_slices, self.R
        ins, outs, results, keep = (_TtiIn * n)(), (_TtiOut * (n * m))(), [], []
        col = sent_col = None
        if column is not None:
            dtype, ctype, tail = self._COLUMNS[column]
            col = (C.POINTER(ctype) * n)()
        if sent:
            sent_col = (C.POINTER(C.c_int32) * n)()
        for k, kw in enumerate(calls):
            kw = dict(kw)
            if update_only and kw.get("n_users", None) == 0:  # (ins[k] stays zero: no users, the cell's update alone)
                if len(kw) != 1:
                    raise AssertionError("an update-only slot gives nothing but n_users=0")
                z = np.zeros(0, np.int32)
                res = TtiResult(np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(R, np.int32), z, z.copy(), z.copy(), z.copy())
                outs[k] = _TtiOut(_p(res.target_rbs, C.c_int32), _p(res.quota_rbgs, C.c_int32), _p(res.rbg_to_user, C.c_int32))
                if sent:
                    res.sent = np.zeros((0, 2), np.int32)
                results.append(res)
                continue
            if column is not None:
                x = np.ascontiguousarray(kw.pop(column), dtype)
            cqi, avg = kw.pop("cqi", None), kw.pop("avg_rate") if need_avg else kw.pop("avg_rate", None)
            row = []
            for j in range(m):  # (a run: one rs_tti_out per TTI; the rs_tti_in is the first one's)
                tin, tout, res, arrays = _marshal_tti(S, R, self.rbg_size, self.sched, cqi, avg, **kw)
                if j == 0:
                    ins[k] = tin
                outs[k * m + j] = tout
                row.append(res)
                keep.append(arrays)
            results.append(res if T is None else row[:T])
            if column is not None:
                if x.shape != (tin.n_users,) + tail:
                    raise AssertionError(f"{column} of shape {x.shape} for {tin.n_users} users")
                col[k] = _p(x, ctype)
                keep.append(x)
            if sent:
                res.sent = np.zeros((tin.n_users, 2), np.int32)
                sent_col[k] = _p(res.sent, C.c_int32)
        t = None if now is _NO_CLOCK else np.ascontiguousarray(np.broadcast_to(np.asarray(now, np.float64), (n,) if T is None else (n, T)))
        ids = _opt(cell_ids, np.int32, (n,))
        keep += [t, ids]
        return _GroupCall(n, _p(ids, C.c_int32), ins, outs, _p(t, C.c_double), col, sent_col, results, keep)

    def schedule_tti(self, calls: Sequence[dict], cell_ids: Optional[Sequence[int]] = None) -> List[TtiResult]:
        """calls[k]: the keyword arguments of TtiScheduler.schedule_tti for cell cell_ids[k] (None: cell k).  Optional inputs are
        given by every cell of a call or by none (a mixed call raises, nothing is launched).  cqi_epoch counts per cell: a cell whose
        call repeats the number, users and kind of report of its last stored call is served from its device-resident image."""
        c = self._marshal(calls, cell_ids, need_avg=True)
        _check(lib().rs_group_schedule_tti(self._h, c.n, c.ids, c.ins, c.outs))
        return c.results

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
        c = self._marshal(calls, cell_ids, now)
        _check(lib().rs_group_schedule_tti_at(self._h, c.n, c.ids, c.ins, c.outs, c.now))
        return c.results

    def run_at(self, calls: Sequence[dict], now, rands=None, cell_ids: Optional[Sequence[int]] = None) -> List[List[TtiResult]]:
        """rs_group_run_at: T consecutive schedule_tti_at calls in one launch.  calls[k] as for schedule_tti_at, given once per cell
        (rand0 / rand1 are not read); now is [T] (the same clock for every cell) or [n][T]; rands is [n][T][2], the rand() pair of each
        cell's TTIs (None: RS_SCHED_PF only).  Returns results[k][t]."""
        return self._run(lib().rs_group_run_at, calls, now, rands, cell_ids, True)

    def _run(self, fn, calls, now, rands, cell_ids, outputs, rec=None):
        """rec: (rec_cap, recs, n_recs) -- the three extra arguments of rs_group_run_records_at (arrays, or None for a NULL pointer)"""
        n = len(calls)
        t = np.asarray(now, np.float64)
        if t.ndim not in (1, 2) or (t.ndim == 2 and t.shape[0] != n):
            raise AssertionError("now is neither [T] nor [n][T]")
        T = t.shape[-1]
        r = _opt(rands, np.int32, (n, T, 2))
        c = self._marshal(calls, cell_ids, t, T)
        more = () if rec is None else (int(rec[0]), None if rec[1] is None else rec[1].ctypes.data, _p(rec[2], C.c_int32))
        _check(fn(self._h, n, c.ids, c.ins, T, c.now, _p(r, C.c_int32), c.outs if outputs else None, *more))
        return c.results if outputs else None

    def _set_counters(self, fn, cell, shape, cum_bytes, cum_rbs, *first):
        """the counter setters: `first` (set_flows' bearers), then cum_bytes and cum_rbs of this shape or NULL"""
        cb, cr = _opt(cum_bytes, np.int64, shape), _opt(cum_rbs, np.int64, shape)
        _check(fn(self._h, cell, *first, _p(cb, C.c_int64), _p(cr, C.c_int64)))

    def _get_counters(self, fn, cell, shape, *first):
        cb, cr = np.zeros(shape, np.int64), np.zeros(shape, np.int64)
        _check(fn(self._h, cell, *first, _p(cb, C.c_int64), _p(cr, C.c_int64)))
        return cb, cr

    # ---- counted runs: m_cumulateBytes / m_cumulateRBs per user of an average-resident cell stay on the device too ----
    def set_avg_counters(self, cell, cum_bytes=None, cum_rbs=None):
        """rs_group_set_avg_counters: makes an average-resident `cell` avg-counted with cum_bytes / cum_rbs int64 [n_users] by user id
        (None: zeros).  Any time between two calls; outside the fast path."""
        self._set_counters(lib().rs_group_set_avg_counters, cell, (self.slices.n_users,), cum_bytes, cum_rbs)

    def get_avg_counters(self, cell):
        """(cum_bytes int64 [n_users], cum_rbs int64 [n_users]) of an avg-counted cell: a synchronising copy, not part of a TTI."""
        return self._get_counters(lib().rs_group_get_avg_counters, cell, (self.slices.n_users,))

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
        c = self._marshal(calls, cell_ids, now, update_only=True, column="data_to_transmit", sent=counted)
        if counted:
            _check(lib().rs_group_schedule_tti_counted(self._h, c.n, c.ids, c.ins, c.outs, c.now, c.column, c.sent))
        else:
            _check(lib().rs_group_schedule_tti_queued(self._h, c.n, c.ids, c.ins, c.outs, c.now, c.column))
        return c.results

    # ---- counted bearers: m_cumulateBytes / m_cumulateRBs of a bearer-resident cell stay on the device too ----
    def set_counters(self, cell, cum_bytes=None, cum_rbs=None):
        """rs_group_set_counters: makes a bearer-resident `cell` counted with cum_bytes / cum_rbs int64 [n_users][2] by user id and
        bearer priority (None: zeros).  Any time between two calls; outside the fast path."""
        self._set_counters(lib().rs_group_set_counters, cell, (self.slices.n_users, 2), cum_bytes, cum_rbs)

    def get_counters(self, cell):
        """(cum_bytes int64 [n_users][2], cum_rbs int64 [n_users][2]) of a counted cell: a synchronising copy, not part of a TTI."""
        return self._get_counters(lib().rs_group_get_counters, cell, (self.slices.n_users, 2))

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
        assert h.shape == (U, 2) and a.shape == (U, 2)
        self._set_counters(lib().rs_group_set_flows, cell, (U, 2), cum_bytes, cum_rbs, _p(h, C.c_uint8), _p(a, C.c_double), float(last_update))

    def get_flows(self, cell):
        """(avg float64, pending bytes int32, last_update, cum_bytes int64, cum_rbs int64) of a flow-resident cell, the arrays
        [n_users][2] and 0 for a bearer that does not exist: a synchronising copy, not part of a TTI."""
        U = self.slices.n_users
        a, pend = np.zeros((U, 2), np.float64), np.zeros((U, 2), np.int32)
        last = C.c_double(0)
        cb, cr = self._get_counters(lib().rs_group_get_flows, cell, (U, 2), _p(a, C.c_double), _p(pend, C.c_int32), C.byref(last))
        return a, pend, float(last.value), cb, cr

    def schedule_tti_flows(self, calls: Sequence[dict], now, cell_ids: Optional[Sequence[int]] = None) -> List[TtiResult]:
        """rs_group_schedule_tti_flows: one TTI of flow-resident cells.  calls[k]: dict(user_id [n], flow_bearer [n] (0 or 1),
        data_to_transmit [n] (> 0), cqi [n][R] or cqi_prb [n][R * rbg_size], cqi_epoch) -- position i is bearer flow_bearer[i] of user
        user_id[i] (None: user i), the pairs ascending; or dict(n_users=0), an update-only slot.  Results are per position, and
        rbg_to_user holds flow ids 2 * user + bearer; the bytes credited to position i are user_tbs_bits[i] // 8."""
        c = self._marshal(calls, cell_ids, now, update_only=True, column="flow_bearer")
        _check(lib().rs_group_schedule_tti_flows(self._h, c.n, c.ids, c.ins, c.outs, c.now, c.column))
        return c.results

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
        self.device = int(device)
        self._cfg = _CfgHolder(slices, n_rbgs, rbg_size, sched, device, stream, synthetic_exp, link_tables)
        bc = _BatchConfig(self._cfg.c, n_cells, first_tti, cqi_refresh, int(phy_error_draws), threads_per_cell,
                          int(jit), int(bool(cqi_epoch_wrap)), int(queue_state_lds), int(bool(autotune)), int(selfcheck))
        self._h = lib().rs_batch_create_checked(C.byref(bc), RS_ABI_VERSION, C.sizeof(_BatchConfig))
        if not self._h:
            raise RadioSaberError(-1, lib().rs_last_error().decode())

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self, "_cqi_in_flight", None):  # tensors of asynchronous writes: released once the stream has passed their packs
                lib().rs_batch_sync(self._h)
                self._cqi_in_flight = []
            lib().rs_batch_destroy(self._h)
            self._h = None

    __del__ = close

    def seed(self, seeds, rand_skip=None):
        s = np.ascontiguousarray(seeds, np.uint32)
        assert s.shape == (self.n_cells,)
        k = _opt(rand_skip, np.int64)
        _check(lib().rs_batch_seed(self._h, _p(s, C.c_uint32), _p(k, C.c_int64)))

    def set_cell_configs(self, configs: Sequence[SliceConfig]):
        """One SliceConfig per cell, of at most the batch's n_slices and n_users: cell c takes configs[c]'s weights, algo_epsilon,
        algo_psi and slice sizes and then runs, to the bit, like a one-cell batch created from configs[c]
        (rs_batch_set_cell_configs_n).  A configuration of fewer users than the batch's makes a cell of that many: its map is padded
        with RS_USER_ABSENT, the users behind it are never served and their state words never touched (cell_users() returns the
        counts; state() and run_logged() keep their [cells][U] shapes).  A configuration of fewer slices makes a cell of that many:
        its weights are padded with 0 and its exponents with 1, the slices behind it take part in nothing and their slice_state words
        are never touched (cell_slices() returns the counts; the [cells][S] shapes stay).  Before the first TTI; never with the
        queue model or scheduler 11.  algo_alpha / algo_beta stay the batch's."""
        if len(configs) != self.n_cells:
            raise ValueError(f"{len(configs)} configurations for {self.n_cells} cells")
        for c, cfg in enumerate(configs):
            if not 1 <= cfg.n_slices <= self.S or not 1 <= cfg.n_users <= self.U:
                raise ValueError(f"configuration {c} has {cfg.n_slices} slices and {cfg.n_users} users, the batch {self.S} and {self.U}")
            k = cfg.n_slices
            if list(cfg.algo_alpha) != list(self.slices.algo_alpha)[:k] or list(cfg.algo_beta) != list(self.slices.algo_beta)[:k]:
                raise ValueError(f"configuration {c} has algo_alpha / algo_beta of its own: the two stay the batch's")
        pad = lambda v, fill: list(v) + [fill] * (self.S - len(v))
        n = np.ascontiguousarray([cfg.n_slices for cfg in configs], np.int32)
        w = np.ascontiguousarray([pad(cfg.weight, 0.0) for cfg in configs], np.float64)
        e = np.ascontiguousarray([pad(cfg.algo_epsilon, 1) for cfg in configs], np.int32)
        p = np.ascontiguousarray([pad(cfg.algo_psi, 1) for cfg in configs], np.int32)
        m = self.padded_maps(configs, self.U)
        # (a batch whose configurations all have its n_slices makes the call it always made)
        if (n == self.S).all():
            _check(lib().rs_batch_set_cell_configs(self._h, _p(w, C.c_double), _p(e, C.c_int32), _p(p, C.c_int32), _p(m, C.c_int32)))
        else:
            _check(lib().rs_batch_set_cell_configs_n(self._h, _p(n, C.c_int32), _p(w, C.c_double), _p(e, C.c_int32), _p(p, C.c_int32),
                                                     _p(m, C.c_int32)))

    @staticmethod
    def padded_maps(configs, n_users):
        """int32 [len(configs)][n_users]: every configuration's user_to_slice, padded with RS_USER_ABSENT to the batch's user count."""
        m = np.full((len(configs), n_users), RS_USER_ABSENT, np.int32)
        for c, cfg in enumerate(configs):
            m[c, :cfg.n_users] = cfg.user_to_slice
        return m

    def cell_users(self):
        """int32 [n_cells]: every cell's user count (rs_batch_cell_users) -- the batch's n_users but for the cells that set_cell_configs
        gave a configuration of fewer users."""
        n = np.zeros(self.n_cells, np.int32)
        _check(lib().rs_batch_cell_users(self._h, _p(n, C.c_int32)))
        return n

    def cell_slices(self):
        """int32 [n_cells]: every cell's slice count (rs_batch_cell_slices) -- the batch's n_slices but for the cells that
        set_cell_configs gave a configuration of fewer slices."""
        n = np.zeros(self.n_cells, np.int32)
        _check(lib().rs_batch_cell_slices(self._h, _p(n, C.c_int32)))
        return n

    def cell_config(self, cell):
        """The configuration cell `cell` runs: dict(weight f64[S], algo_epsilon, algo_psi i32[S], user_to_slice i32[U])
        (rs_batch_get_cell_config; the shared configuration's rows where set_cell_configs was never called)."""
        w, e, p = np.zeros(self.S, np.float64), np.zeros(self.S, np.int32), np.zeros(self.S, np.int32)
        m = np.zeros(self.U, np.int32)
        _check(lib().rs_batch_get_cell_config(self._h, int(cell), _p(w, C.c_double), _p(e, C.c_int32), _p(p, C.c_int32), _p(m, C.c_int32)))
        return {"weight": w, "algo_epsilon": e, "algo_psi": p, "user_to_slice": m}

    def slice_totals(self):
        """{"cum_bytes", "cum_rbs"}: int64 [n_cells][S], every cell's per-user counters summed by the cell's own slice map on the
        device (rs_batch_slice_totals)."""
        cb = np.zeros((self.n_cells, self.S), np.int64)
        cr = np.zeros((self.n_cells, self.S), np.int64)
        _check(lib().rs_batch_slice_totals(self._h, _p(cb, C.c_int64), _p(cr, C.c_int64)))
        return {"cum_bytes": cb, "cum_rbs": cr}

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

    # ---- epoch grids from device memory (rs_pack_cqi_kernel on the batch's stream) ----
    def _device_grids(self, t, what):
        """(t's address, its byte count, its epoch count) of a torch uint8 tensor [n_cells, E, U, R] on the batch's device, contiguous
        (a view that begins at any byte of a larger tensor will do); ValueError for anything else, before any C call.  Duck-typed:
        torch is not imported for the checks."""
        for attr in ("data_ptr", "is_cuda", "is_contiguous", "element_size", "shape", "device"):
            if not hasattr(t, attr):
                raise ValueError(f"{what}: a torch tensor on the batch's device is needed, not {type(t).__name__}")
        if not t.is_cuda:
            raise ValueError(f"{what}: the tensor is on {t.device}, not on the batch's device {self.device}")
        index = t.device.index
        if index is not None and int(index) != self.device:
            raise ValueError(f"{what}: the tensor is on device {index}, the batch on device {self.device}")
        if t.element_size() != 1 or not str(t.dtype).endswith("uint8"):
            raise ValueError(f"{what}: dtype {t.dtype}, uint8 is needed")
        shape = tuple(int(x) for x in t.shape)
        if len(shape) != 4 or shape[0] != self.n_cells or shape[1] < 1 or shape[2:] != (self.U, self.R):
            raise ValueError(f"{what}: shape {shape}, [{self.n_cells}, E, {self.U}, {self.R}] is needed")
        if not t.is_contiguous():
            raise ValueError(f"{what}: the tensor is not contiguous")
        return int(t.data_ptr()), shape[0] * shape[1] * shape[2] * shape[3], shape[1]

    def _after_torch_stream(self, t):
        """the batch's stream, as torch sees it, made to wait for what torch's current stream has enqueued so far (the producer of t)"""
        import torch
        s = torch.cuda.ExternalStream(self.stream or 0, device=t.device)
        s.wait_stream(torch.cuda.current_stream(t.device))
        return s

    def _keep_until_packed(self, s, t):
        """An asynchronous write reads t after the call has returned: the batch holds t until an event behind the pack has completed,
        so that the caching allocator cannot hand its memory out again before.  (Not Tensor.record_stream: the allocator would then
        record an event on the batch's stream when the tensor is freed, which may be after close() has destroyed that stream.)"""
        import torch
        done = torch.cuda.Event()
        done.record(s)
        self._cqi_in_flight = [(e, x) for e, x in getattr(self, "_cqi_in_flight", ()) if not e.query()] + [(done, t)]

    def set_cqi_epochs_device(self, t):
        """upload_cqi_epochs from a torch uint8 tensor [n_cells, E, U, R] on the batch's device: packed, checked and clamped by a
        kernel on the batch's stream, behind what torch's current stream has enqueued; returns when it is done
        (rs_batch_set_cqi_epochs_device).  A value outside 1..15 raises RadioSaberError and leaves the batch without a CQI source."""
        ptr, nbytes, n_epochs = self._device_grids(t, "set_cqi_epochs_device")
        self._after_torch_stream(t)
        _check(lib().rs_batch_set_cqi_epochs_device(self._h, ptr, nbytes, n_epochs))
        self.n_epochs = n_epochs

    def write_cqi_epochs_device(self, first_epoch, t, sync=True):
        """Rewrites epochs first_epoch .. first_epoch + E - 1 (modulo n_epochs with cqi_epoch_wrap) of the grids on the device from
        t = [n_cells, E, U, R], in place, on the batch's stream: behind the launches made so far and ahead of the later ones
        (rs_batch_write_cqi_epochs_device).  sync=False returns after the enqueue (RS_CQI_WRITE_ASYNC): values outside 1..15 then run
        as CQI 1 and cqi_write_status() reports them; the batch keeps t alive until the pack has read it."""
        ptr, nbytes, n = self._device_grids(t, "write_cqi_epochs_device")
        s = self._after_torch_stream(t)
        _check(lib().rs_batch_write_cqi_epochs_device(self._h, int(first_epoch), n, ptr, nbytes, 0 if sync else RS_CQI_WRITE_ASYNC))
        if not sync:
            self._keep_until_packed(s, t)

    def cqi_write_status(self):
        """Waits for the batch's stream; None when no pack since the last report met a value outside 1..15, else (byte index in its
        call's tensor, value) of the lowest such byte -- the report then leaves the batch without a CQI source
        (rs_batch_cqi_write_status)."""
        byte, value = C.c_int64(-1), C.c_int32(0)
        rc = lib().rs_batch_cqi_write_status(self._h, C.byref(byte), C.byref(value))
        if rc == -1 and byte.value >= 0:
            return int(byte.value), int(value.value)
        _check(rc)
        return None

    def debug_cqi_image(self, cell, epoch):
        """uint8 [round_up(Upad * R, 16)]: one grid exactly as stored, [R][Upad] with its zero padding and tail (rs_batch_debug_cqi_image)"""
        k = (self.U + 7) // 8
        upad = 8 * (k if k & 1 else k + 1)
        out = np.zeros((upad * self.R + 15) // 16 * 16, np.uint8)
        _check(lib().rs_batch_debug_cqi_image(self._h, int(cell), int(epoch), _p(out, C.c_uint8), out.size))
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
                       _p(keys, C.c_uint32))
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

    def grant_bound(self):
        """rs_batch_grant_bound: the most grants one cell can get in one TTI (backlogged batches; schedulers other than 11)."""
        return _count(lib().rs_batch_grant_bound(self._h))

    def run_grant_records(self, n_ttis, cap=None, out=None):
        """run(n_ttis) that also returns, per cell, a BATCH_GRANT_RECORD array with one record per (TTI, user) DoStopSchedule credited
        in these TTIs, ascending in TTI, then in user: the order of the log's lines (rs_batch_run_grant_records; what
        logfmt.grant_record_lines reads).  cap: the places per cell, default n_ttis * grant_bound(), which cannot overflow.  A cell that
        counts more than cap raises RadioSaberError (RS_ERR_RANGE) after the launch has completed; the error carries .records (the lists
        as far as they were written) and .counts (the counts as counted).  out: a BATCH_GRANT_RECORD array [n_cells][cap] of an earlier
        call to write into (the returned lists are views of it): a caller that launches again and again spares the host the page faults
        of a fresh block."""
        if cap is None:
            cap = max(int(n_ttis), 1) * self.grant_bound() if out is None else out.shape[1]
        if out is not None and (out.dtype != BATCH_GRANT_RECORD or out.shape != (self.n_cells, int(cap)) or not out.flags.c_contiguous):
            raise ValueError("out is not a C-contiguous BATCH_GRANT_RECORD array of shape (n_cells, cap)")
        recs = np.zeros((self.n_cells, max(int(cap), 1)), BATCH_GRANT_RECORD) if out is None else out
        n = np.zeros(self.n_cells, np.int64)
        rc = lib().rs_batch_run_grant_records(self._h, n_ttis, cap, recs.ctypes.data_as(C.c_void_p), _p(n, C.c_int64))
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
        a = _opt(avg_rate, np.float64, (self.n_cells, self.U))
        s = _opt(slice_state, np.float64, (self.n_cells, self.S))
        _check(lib().rs_batch_write_state(self._h, _p(a, C.c_double), _p(s, C.c_double)))

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
