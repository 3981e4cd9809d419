"""ctypes binding of libra_gpu_batch.so (the C ABI of include/ra_gpu_batch.h).

This is exactly what the Erlang NIF binds (ra_amd/csrc/ra_gpu_batch_nif.c); Python plays the
role of the gen_statem shell in tests and benchmarks.  No CPU fallback: a missing library or a
missing GPU raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from . import abi

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB_PATH = os.environ.get("RGB_LIB") or os.path.join(_CSRC, "libra_gpu_batch.so")

EXPORTS = [
    "rgb_abi_version", "rgb_struct_size", "rgb_strerror", "rgb_default_config", "rgb_open",
    "rgb_close", "rgb_last_hip_error", "rgb_register_groups", "rgb_n_servers", "rgb_upload_state",
    "rgb_download_state", "rgb_submit", "rgb_collect", "rgb_run_ticks_device", "rgb_snapshot",
    "rgb_snapshot_device", "rgb_state_checksum", "rgb_synchronize", "rgb_wait", "rgb_wake", "rgb_in_flight",
    "rgb_route", "rgb_submit_trains", "rgb_peek",
    "rgb_train_bucket", "rgb_train_plan_create", "rgb_train_plan_destroy", "rgb_train_plan_blocks_per_tick",
    "rgb_train_stamp_device", "rgb_train_run_device", "rgb_train_status", "rgb_train_form", "rgb_train_recoveries",
    "rgb_train_plan_create_snap", "rgb_train_run_snap_device", "rgb_snapshot_train_device", "rgb_train_seq_bytes",
    "rgb_train_plan_create_device", "rgb_train_plan_build_device", "rgb_train_plan_download", "rgb_train_plan_fit",
    "rgb_submit_seq", "rgb_set_seq_ranges_device", "rgb_collect_view", "rgb_release",
    "rgb_submit_raw_capacity", "rgb_submit_begin", "rgb_submit_commit", "rgb_submit_raw",
]
COMM_EXPORTS = ["rgb_comm_unique_id", "rgb_comm_init_rank", "rgb_comm_destroy", "rgb_comm_n_ranks", "rgb_comm_rank",
                "rgb_leaderboard_allgather", "rgb_leaderboard_allgather_host", "rgb_comm_last_error"]   # the one collective of the path (RCCL)
EXPORTS += COMM_EXPORTS
SYNTH_EXPORTS = ["rgb_synth_tick_device", "rgb_synth_tick_buckets_device", "rgb_synth_apply_tick_device",
                 "rgb_synth_tick_stamped_device", "rgb_synth_stamps_resync_device",
                 "rgb_synth_snapshot_mark_device", "rgb_synth_set_hint"]                                       # include/ra_gpu_batch_synth.h (bench tooling)
OPTIONAL_IN_OLD_BUILDS = {"rgb_synth_tick_stamped_device", "rgb_synth_stamps_resync_device", "rgb_train_form",
                          "rgb_train_recoveries", "rgb_train_plan_create_snap", "rgb_train_run_snap_device",
                          "rgb_snapshot_train_device", "rgb_train_seq_bytes", "rgb_synth_snapshot_mark_device",
                          "rgb_synth_set_hint", "rgb_train_plan_create_device", "rgb_train_plan_build_device",
                          "rgb_train_plan_download", "rgb_train_plan_fit", "rgb_submit_seq", "rgb_set_seq_ranges_device",
                          "rgb_collect_view", "rgb_release", "rgb_submit_raw_capacity", "rgb_submit_begin",
                          "rgb_submit_commit", "rgb_submit_raw"} | set(COMM_EXPORTS)
WAL_EXPORTS = ["rgb_wal_adler32_device", "rgb_wal_adler32", "rgb_wal_layout", "rgb_wal_frame_device",
               "rgb_wal_frame", "rgb_wal_scan", "rgb_wal_validate",
               "rgb_wal_batch_bound", "rgb_wal_batch_device", "rgb_wal_batch",
               "rgb_crc32_device", "rgb_crc32", "rgb_crc32_stream_device", "rgb_crc32_stream", "rgb_segment_layout",
               "rgb_segment_build_device", "rgb_segment_build", "rgb_segment_scan", "rgb_segment_validate",
               "rgb_segment_compact_bound", "rgb_segment_info_device", "rgb_segment_info", "rgb_segment_compact_device",
               "rgb_segment_compact", "rgb_segment_compact_select", "rgb_segment_compact_take_groups",
               "rgb_segment_compact_groups_bound", "rgb_segment_compact_groups_device", "rgb_segment_compact_groups",
               "rgb_segment_flush_bound", "rgb_segment_flush_device", "rgb_segment_flush",
               "rgb_segment_read_device", "rgb_segment_read",
               "rgb_crc32_spans_device", "rgb_crc32_spans", "rgb_snapshot_layout", "rgb_snapshot_build_device",
               "rgb_snapshot_build", "rgb_snapshot_validate_device", "rgb_snapshot_validate"]                                                                                 # include/ra_gpu_wal.h


class RgbError(RuntimeError):
    def __init__(self, code: int, what: str, hip: int = 0):
        self.code, self.hip = code, hip
        super().__init__(f"{what}: rc={code} ({_strerror(code)})" + (f" hipError={hip}" if hip else ""))


def build(force: bool = False) -> str:
    """Compile the HIP library for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(_CSRC, f) for f in ("rgb_kernels.hip", "rgb_api.hip", "rgb_prepare.hip", "rgb_wal.hip", "rgb_wal_host.cpp", "rgb_segment.hip",
                                              "rgb_segment_host.cpp", "rgb_comm.cpp", "rgb_internal.h")]
    srcs.append(os.path.join(_CSRC, "..", "..", "include", "ra_gpu_wal.h"))
    srcs.append(os.path.join(_CSRC, "..", "..", "include", "ra_gpu_batch.h"))
    stale = (not os.path.exists(LIB_PATH)) or any(
        os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if force or stale:
        subprocess.check_call(["make", "-C", _CSRC, "libra_gpu_batch.so"])
    return LIB_PATH


_lib = None


def lib():
    """Load the library and verify the ABI.  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it (python -c 'import __graft_entry__ as g; g.build()' "
            "or make -C ra_amd/csrc).  ra_gpu_batch has no CPU fallback.")
    # One HIP/HSA runtime per process: when PyTorch is installed its bundled libamdhip64.so.7 must
    # be the copy in the process (a second HSA runtime cannot open the device), so import torch
    # BEFORE the library resolves that soname.  The library itself has no torch dependency (the
    # Erlang NIF uses /opt/rocm's runtime).
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is optional for the binding
        pass
    L = C.CDLL(LIB_PATH)
    for name in EXPORTS + SYNTH_EXPORTS + WAL_EXPORTS:
        if not hasattr(L, name):
            # tools/ only: RGB_LIB=<an older build> for same-box A/B timing of bench.py (tools/gpu_ab.sh --variants)
            if os.environ.get("RGB_LIB") and name in OPTIONAL_IN_OLD_BUILDS:
                continue
            raise RuntimeError(f"libra_gpu_batch.so does not export {name}")
    vp, u32, u64p = C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)
    L.rgb_abi_version.restype = C.c_uint32
    L.rgb_struct_size.restype = C.c_size_t
    L.rgb_struct_size.argtypes = [C.c_int]
    L.rgb_strerror.restype = C.c_char_p
    L.rgb_strerror.argtypes = [C.c_int]
    L.rgb_default_config.argtypes = [vp]
    L.rgb_open.argtypes = [vp, C.POINTER(vp)]
    L.rgb_close.argtypes = [vp]
    L.rgb_last_hip_error.argtypes = [vp]
    L.rgb_register_groups.argtypes = [vp, u32, u32]
    L.rgb_n_servers.restype = C.c_uint32
    L.rgb_n_servers.argtypes = [vp]
    L.rgb_upload_state.argtypes = [vp, u32, u32, vp]
    L.rgb_download_state.argtypes = [vp, u32, u32, vp]
    L.rgb_submit.argtypes = [vp, vp, u32, C.c_uint64]
    if hasattr(L, "rgb_submit_seq"):
        L.rgb_submit_seq.argtypes = [vp, vp, u32, C.c_uint64, vp, u32]
        L.rgb_set_seq_ranges_device.argtypes = [vp, vp, u32]
    L.rgb_collect.argtypes = [vp, vp, u32, C.POINTER(u32), vp, u32, C.POINTER(u32), u64p]
    if hasattr(L, "rgb_collect_view"):
        L.rgb_collect_view.argtypes = [vp, vp]
        L.rgb_release.argtypes = [vp, u32]
    if hasattr(L, "rgb_submit_raw"):
        L.rgb_submit_raw_capacity.restype = C.c_uint32
        L.rgb_submit_raw_capacity.argtypes = [vp, u32]
        L.rgb_submit_begin.argtypes = [vp, u32, vp]
        L.rgb_submit_commit.argtypes = [vp, u32, u32, C.c_uint64]
        L.rgb_submit_raw.argtypes = [vp, vp, u32, u32, C.c_uint64]
    L.rgb_run_ticks_device.argtypes = [vp, vp, u32, vp, vp, vp, u32, vp, vp, vp]
    L.rgb_snapshot.argtypes = [vp, vp]
    L.rgb_snapshot_device.argtypes = [vp, vp, vp]
    L.rgb_state_checksum.argtypes = [vp, u32, u32, u64p]
    L.rgb_synchronize.argtypes = [vp]
    L.rgb_wait.argtypes = [vp, u32]
    L.rgb_wake.argtypes = [vp]
    L.rgb_wake.restype = None
    L.rgb_in_flight.argtypes = [vp]
    L.rgb_peek.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)]
    L.rgb_submit_trains.restype = C.c_uint32
    L.rgb_submit_trains.argtypes = [vp]
    L.rgb_in_flight.restype = C.c_uint32
    L.rgb_route.argtypes = [C.c_uint64, u32]
    L.rgb_route.restype = C.c_uint32
    L.rgb_synth_tick_device.argtypes = [vp, C.c_uint64, C.c_uint64, vp, vp, vp, vp]
    L.rgb_synth_tick_buckets_device.argtypes = [vp, C.c_uint64, C.c_uint64, vp, vp, vp, vp, vp]
    if hasattr(L, "rgb_synth_tick_stamped_device"):
        L.rgb_synth_tick_stamped_device.argtypes = [vp, C.c_uint64, C.c_uint64, vp, vp, vp, vp, vp, vp]
        L.rgb_synth_stamps_resync_device.argtypes = [vp, vp]
    if hasattr(L, "rgb_comm_init_rank"):
        L.rgb_comm_unique_id.argtypes = [vp]
        L.rgb_comm_init_rank.argtypes = [vp, vp, u32, u32, C.POINTER(vp)]
        L.rgb_comm_destroy.argtypes = [vp]
        L.rgb_comm_destroy.restype = None
        L.rgb_comm_n_ranks.argtypes = [vp]
        L.rgb_comm_n_ranks.restype = C.c_uint32
        L.rgb_comm_rank.argtypes = [vp]
        L.rgb_comm_rank.restype = C.c_uint32
        L.rgb_leaderboard_allgather.argtypes = [vp, vp, vp, u32, vp, vp]
        L.rgb_comm_last_error.restype = C.c_char_p
    if hasattr(L, "rgb_debug_inject_train_fault"):
        L.rgb_debug_inject_train_fault.argtypes = [vp, u32]
        L.rgb_debug_inject_train_fault.restype = None
        L.rgb_train_recoveries.argtypes = [vp]
        L.rgb_train_recoveries.restype = C.c_uint32
        L.rgb_train_form.argtypes = [vp]
        L.rgb_train_form.restype = C.c_uint32
    L.rgb_train_bucket.restype = C.c_uint32
    L.rgb_train_bucket.argtypes = [u32, u32, u32, u32]
    L.rgb_train_plan_create.argtypes = [vp, vp, u32, C.POINTER(vp)]
    L.rgb_train_plan_destroy.argtypes = [vp]
    L.rgb_train_plan_destroy.restype = None
    L.rgb_train_plan_blocks_per_tick.restype = C.c_uint32
    L.rgb_train_plan_blocks_per_tick.argtypes = [vp]
    L.rgb_train_stamp_device.argtypes = [vp, vp, vp, u32, vp, u32, vp]
    L.rgb_train_run_device.argtypes = [vp, vp, u32, u32, vp, vp, u32, vp, vp, u32, vp]
    if hasattr(L, "rgb_train_run_snap_device"):
        L.rgb_train_plan_create_snap.argtypes = [vp, vp, u32, u32, C.POINTER(vp)]
        L.rgb_train_run_snap_device.argtypes = [vp, vp, u32, u32, vp, vp, u32, vp, vp, u32, vp, vp, vp]
        L.rgb_snapshot_train_device.argtypes = [vp, vp, vp]
        L.rgb_train_seq_bytes.restype = C.c_uint32
        L.rgb_train_seq_bytes.argtypes = [vp]
        L.rgb_synth_snapshot_mark_device.argtypes = [vp, vp, vp]
    if hasattr(L, "rgb_train_plan_create_device"):          # ABI v8
        L.rgb_train_plan_create_device.argtypes = [vp, u32, u32, C.POINTER(vp)]
        L.rgb_train_plan_build_device.argtypes = [vp, vp, u32, u32, vp, vp]
        L.rgb_train_plan_download.argtypes = [vp, vp, u32, vp, vp, u32]
    if hasattr(L, "rgb_train_plan_fit"):
        L.rgb_train_plan_fit.argtypes = [vp, vp, u32, u32, vp]
    L.rgb_train_status.argtypes = [vp, C.POINTER(u32), vp]
    L.rgb_synth_apply_tick_device.argtypes = [vp, vp, u32, vp, vp, vp]
    if hasattr(L, "rgb_synth_set_hint"):
        L.rgb_synth_set_hint.argtypes = [vp, u32]
    L.rgb_wal_adler32_device.argtypes = [vp, vp, u32, vp, C.c_uint64, vp, vp]
    L.rgb_wal_adler32.argtypes = [vp, vp, u32, vp, C.c_uint64, vp]
    L.rgb_wal_layout.restype = C.c_uint64
    L.rgb_wal_layout.argtypes = [vp, u32, C.c_uint64]
    L.rgb_wal_frame_device.argtypes = [vp, vp, u32, vp, C.c_uint64, vp, C.c_uint64, vp, u32, vp]
    L.rgb_wal_frame.argtypes = [vp, vp, u32, vp, C.c_uint64, vp, C.c_uint64, u32]
    L.rgb_wal_scan.argtypes = [vp, C.c_uint64, vp, u32, C.POINTER(C.c_uint32), u64p, C.POINTER(C.c_uint32)]
    L.rgb_wal_validate.argtypes = [vp, vp, C.c_uint64, vp, u32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    u32p = C.POINTER(C.c_uint32)
    L.rgb_crc32_device.argtypes = [vp, vp, u32, vp, C.c_uint64, vp, vp]
    L.rgb_crc32.argtypes = [vp, vp, u32, vp, C.c_uint64, vp]
    L.rgb_crc32_stream_device.argtypes = [vp, vp, C.c_uint64, u32, vp, vp]
    L.rgb_crc32_stream.argtypes = [vp, vp, C.c_uint64, u32, u32p]
    L.rgb_segment_layout.restype = C.c_uint64
    L.rgb_segment_layout.argtypes = [vp, u32, u32, vp]
    L.rgb_segment_build_device.argtypes = [vp, vp, u32, u32, vp, vp, C.c_uint64, vp, C.c_uint64, u32, vp]
    L.rgb_segment_build.argtypes = [vp, vp, u32, u32, vp, C.c_uint64, vp, C.c_uint64, u32]
    L.rgb_segment_scan.argtypes = [vp, C.c_uint64, vp, u32, u32p, u32p, u32p, u32p]
    L.rgb_segment_validate.argtypes = [vp, vp, C.c_uint64, vp, u32, u32p]
    L.rgb_segment_compact_bound.argtypes = [vp, u32, vp, u32, C.c_uint64, u64p, u32p]
    L.rgb_segment_info_device.argtypes = [vp, vp, u32, vp, C.c_uint64, vp, u32, vp, vp]
    L.rgb_segment_info.argtypes = [vp, vp, u32, vp, C.c_uint64, vp, u32, vp]
    L.rgb_segment_compact_device.argtypes = [vp, vp, u32, vp, C.c_uint64, vp, u32, C.c_uint64, u32, vp, C.c_uint64, vp, vp]
    L.rgb_segment_compact.argtypes = [vp, vp, u32, vp, C.c_uint64, vp, u32, C.c_uint64, u32, vp, C.c_uint64, vp]
    L.rgb_segment_compact_select.argtypes = [vp, u32, vp, u32, vp, u32, vp, vp, u32, u32p]
    L.rgb_segment_compact_take_groups.argtypes = [vp, u32, vp, vp, u32, C.c_uint64, C.c_uint64, vp]
    L.rgb_segment_compact_groups_bound.argtypes = [vp, u32, vp, u32, vp, u32, C.c_uint64, u64p, vp]
    L.rgb_segment_compact_groups_device.argtypes = [vp, vp, u32, vp, u32, vp, C.c_uint64, vp, u32, C.c_uint64, u32, vp,
                                                    C.c_uint64, vp, vp]
    L.rgb_segment_compact_groups.argtypes = [vp, vp, u32, vp, u32, vp, C.c_uint64, vp, u32, C.c_uint64, u32, vp,
                                             C.c_uint64, vp]
    L.rgb_wal_batch_bound.argtypes = [vp, u32, vp, u32, vp, C.c_uint64, u64p, u32p, u32p]
    L.rgb_wal_batch_device.argtypes = [vp, vp, u32, vp, u32, vp, vp, C.c_uint64, u32, vp, vp, vp, C.c_uint64, vp, u32,
                                       vp, u32, vp, vp]
    L.rgb_wal_batch.argtypes = [vp, vp, u32, vp, u32, vp, vp, C.c_uint64, u32, vp, vp, vp, C.c_uint64, vp, u32, vp, u32,
                                vp]
    L.rgb_segment_flush_bound.argtypes = [vp, u32, u32, C.c_uint64, u64p, u32p]
    L.rgb_segment_flush_device.argtypes = [vp, vp, u32, vp, u32, vp, C.c_uint64, u32, C.c_uint64, u32, vp, u32, vp,
                                           C.c_uint64, vp, vp]
    L.rgb_segment_flush.argtypes = [vp, vp, u32, vp, u32, vp, C.c_uint64, u32, C.c_uint64, u32, vp, u32, vp, C.c_uint64, vp]
    L.rgb_segment_read_device.argtypes = [vp, vp, u32, vp, C.c_uint64, vp, u32, u32, vp, vp, C.c_uint64, vp, vp, vp]
    L.rgb_segment_read.argtypes = [vp, vp, u32, vp, C.c_uint64, vp, u32, u32, vp, vp, C.c_uint64, vp, vp]
    L.rgb_crc32_spans_device.argtypes = [vp, vp, u32, vp, C.c_uint64, vp, vp]
    L.rgb_crc32_spans.argtypes = [vp, vp, u32, vp, C.c_uint64, vp]
    L.rgb_snapshot_layout.restype = C.c_uint64
    L.rgb_snapshot_layout.argtypes = [vp, u32, C.c_uint64]
    L.rgb_snapshot_build_device.argtypes = [vp, vp, u32, vp, C.c_uint64, vp, C.c_uint64, vp, vp]
    L.rgb_snapshot_build.argtypes = [vp, vp, u32, vp, C.c_uint64, vp, C.c_uint64, vp]
    L.rgb_snapshot_validate_device.argtypes = [vp, vp, u32, vp, C.c_uint64, vp, vp]
    L.rgb_snapshot_validate.argtypes = [vp, vp, u32, vp, C.c_uint64, vp]
    if L.rgb_abi_version() != abi.ABI_VERSION and not (os.environ.get("RGB_LIB") and L.rgb_abi_version() == abi.ABI_VERSION - 1):
        raise RuntimeError("ABI version mismatch")     # (RGB_LIB=<the previous ABI's build>: A/B timing, tools/ only)
    for i, dt in enumerate(abi.STRUCT_DTYPES):
        if os.environ.get("RGB_LIB") and i >= 6 and L.rgb_abi_version() < abi.ABI_VERSION:
            continue                                       # (an older A/B build has no rgb_view)
        if os.environ.get("RGB_LIB") and i >= 7 and not hasattr(L, "rgb_submit_raw"):
            continue                                       # (.. and the build before the raw submit has no rgb_fill)
        if L.rgb_struct_size(i) != dt.itemsize:
            raise RuntimeError(f"struct {i}: C size {L.rgb_struct_size(i)} != numpy {dt.itemsize}")
    _lib = L
    return L


def _strerror(code: int) -> str:
    try:
        return lib().rgb_strerror(code).decode()
    except Exception:
        return "?"


def default_config() -> np.ndarray:
    cfg = np.zeros(1, dtype=abi.CONFIG_DTYPE)
    lib().rgb_default_config(cfg.ctypes.data)
    return cfg


class RaGpuBatch:
    """One rgb_ctx: the device-resident state of n_groups x n_members ra_servers on one GPU."""

    def __init__(self, n_groups: int, n_members: int, device: int = 0, max_runs: int = 8,
                 ring_slots: int = 4, ring_capacity: int = 65536, max_pipeline_count: int = 0,
                 max_aer_batch: int = 0, flags: int = 0):
        self._L = lib()
        cfg = default_config()
        cfg["device"] = device
        cfg["max_runs"] = max_runs
        cfg["ring_slots"] = ring_slots
        cfg["ring_capacity"] = ring_capacity
        if max_pipeline_count:
            cfg["max_pipeline_count"] = max_pipeline_count
        if max_aer_batch:
            cfg["max_aer_batch"] = max_aer_batch
        cfg["flags"] = flags                    # abi.CFG_SUBMIT_TRAINS: fuse the sub-tick rounds of a batch into a train
        h = C.c_void_p()
        rc = self._L.rgb_open(cfg.ctypes.data, C.byref(h))
        if rc:
            raise RgbError(rc, "rgb_open")
        self._h = h
        self.n_groups, self.n_members = n_groups, n_members
        self.n_servers = n_groups * n_members
        self.ring_capacity = ring_capacity
        self._check(self._L.rgb_register_groups(self._h, n_groups, n_members), "rgb_register_groups")

    # -- plumbing ------------------------------------------------------------------
    def _check(self, rc: int, what: str):
        if rc:
            raise RgbError(rc, what, self._L.rgb_last_hip_error(self._h) if self._h else 0)

    def close(self):
        if getattr(self, "_h", None):
            self._L.rgb_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- state transfer ----------------------------------------------------------------
    def set_state(self, first: int, states: np.ndarray):
        st = np.ascontiguousarray(states, dtype=abi.SERVER_STATE_DTYPE)
        self._check(self._L.rgb_upload_state(self._h, first, len(st), st.ctypes.data), "rgb_upload_state")

    def get_state(self, first: int = 0, n: int | None = None) -> np.ndarray:
        n = self.n_servers - first if n is None else n
        out = np.zeros(n, dtype=abi.SERVER_STATE_DTYPE)
        self._check(self._L.rgb_download_state(self._h, first, n, out.ctypes.data), "rgb_download_state")
        return out

    # -- host path -------------------------------------------------------------------
    def submit(self, msgs: np.ndarray, tick: int = 0, seq_ranges: np.ndarray | None = None):
        """seq_ranges (uint64[n][2]: first, last): the batch's range list -- the lower ranges of written events of more
        than two ranges (abi.MF_SEQX: record fields c = first entry, n_entries = how many) -- rgb_submit_seq."""
        m = np.ascontiguousarray(msgs, dtype=abi.MSG_DTYPE)
        if seq_ranges is None or len(seq_ranges) == 0:
            self._check(self._L.rgb_submit(self._h, m.ctypes.data, len(m), tick), "rgb_submit")
        else:
            r = np.ascontiguousarray(seq_ranges, dtype=np.uint64).reshape(-1, 2)
            self._check(self._L.rgb_submit_seq(self._h, m.ctypes.data, len(m), tick, r.ctypes.data, len(r)), "rgb_submit_seq")

    def collect(self, cap: int | None = None, rpc_cap: int | None = None, out=None):
        """Wait for the oldest submitted batch.  `out` = (decisions, rpcs) preallocated arrays to
        reuse (the NIF hands BEAM binaries instead); returns views of the filled parts."""
        if out is not None:
            dec, rpcs = out
            cap, rpc_cap = len(dec), len(rpcs)
        else:
            cap = self.ring_capacity if cap is None else cap
            rpc_cap = cap * max(self.n_members - 1, 1) if rpc_cap is None else rpc_cap
            dec = np.empty(cap, dtype=abi.DECISION_DTYPE)
            rpcs = np.empty(max(rpc_cap, 1), dtype=abi.RPC_DTYPE)
        n, nr, tick = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
        rc = self._L.rgb_collect(self._h, dec.ctypes.data, cap, C.byref(n), rpcs.ctypes.data,
                                 rpc_cap, C.byref(nr), C.byref(tick))
        if rc in (abi.E_FULL, abi.E_INVAL) and out is None and (n.value > cap or nr.value > rpc_cap):
            # the batch stayed in the ring and reported the sizes it needs: retry once with them
            cap, rpc_cap = max(cap, n.value), max(rpc_cap, nr.value)
            dec = np.empty(max(cap, 1), dtype=abi.DECISION_DTYPE)
            rpcs = np.empty(max(rpc_cap, 1), dtype=abi.RPC_DTYPE)
            rc = self._L.rgb_collect(self._h, dec.ctypes.data, cap, C.byref(n), rpcs.ctypes.data,
                                     rpc_cap, C.byref(nr), C.byref(tick))
        self._check(rc, "rgb_collect")
        return dec[:n.value], rpcs[:nr.value], tick.value

    def collect_view(self):
        """The oldest submitted batch IN PLACE (rgb_collect_view, ABI v9): (decisions, rpcs, tick, slot) where the two
        arrays are numpy views of the pinned slot the device wrote -- no copy.  They are valid until release(slot);
        the slot is not free for rgb_submit before that."""
        v = np.zeros(1, dtype=abi.VIEW_DTYPE)
        self._check(self._L.rgb_collect_view(self._h, v.ctypes.data), "rgb_collect_view")
        n, nr = int(v["n"][0]), int(v["n_rpcs"][0])

        def arr(ptr, count, dt):
            if not count:
                return np.empty(0, dtype=dt)
            buf = (C.c_char * (count * dt.itemsize)).from_address(int(ptr))
            return np.frombuffer(buf, dtype=dt, count=count)
        return arr(v["decisions"][0], n, abi.DECISION_DTYPE), arr(v["rpcs"][0], nr, abi.RPC_DTYPE), int(v["tick"][0]), int(v["slot"][0])

    def release(self, slot: int):
        self._check(self._L.rgb_release(self._h, slot), "rgb_release")

    # -- submitting without the host passes: validation, rounds and bucket order on the device --------
    def raw_capacity(self, max_rounds: int = 4) -> int:
        """Messages a raw batch may hold when no server gets more than max_rounds of them (rgb_submit_raw_capacity)."""
        return int(self._L.rgb_submit_raw_capacity(self._h, max_rounds))

    def submit_raw(self, msgs: np.ndarray, tick: int = 0, max_rounds: int = 4):
        """rgb_submit_raw: the records travel in submission order; what rgb_submit refuses synchronously because of
        the input comes back from collect() / collect_view() instead, once, as the batch's error."""
        m = np.ascontiguousarray(msgs, dtype=abi.MSG_DTYPE)
        self._check(self._L.rgb_submit_raw(self._h, m.ctypes.data, len(m), max_rounds, tick), "rgb_submit_raw")

    def submit_begin(self, max_rounds: int = 4):
        """rgb_submit_begin: (records, slot) -- a numpy view of the slot's pinned message buffer (raw_capacity(max_rounds)
        records) to fill in submission order, and the slot for submit_commit.  Every later commit and submit waits
        for this slot's commit."""
        f = np.zeros(1, dtype=abi.FILL_DTYPE)
        self._check(self._L.rgb_submit_begin(self._h, max_rounds, f.ctypes.data), "rgb_submit_begin")
        cap = int(f["cap"][0])
        buf = (C.c_char * (max(cap, 1) * abi.MSG_DTYPE.itemsize)).from_address(int(f["msgs"][0]))
        return np.frombuffer(buf, dtype=abi.MSG_DTYPE, count=cap), int(f["slot"][0])

    def submit_commit(self, slot: int, n: int, tick: int = 0):
        self._check(self._L.rgb_submit_commit(self._h, slot, n, tick), "rgb_submit_commit")

    def step_raw(self, msgs: np.ndarray, max_rounds: int = 4):
        """submit_raw + collect, in chunks of raw_capacity(max_rounds)."""
        m = np.ascontiguousarray(msgs, dtype=abi.MSG_DTYPE)
        cap = self.raw_capacity(max_rounds)
        out_d, out_r = [], []
        for off in range(0, max(len(m), 1), cap):
            chunk = m[off:off + cap]
            self.submit_raw(chunk, max_rounds=max_rounds)
            d, r, _ = self.collect(cap=max(len(chunk), 1))
            r = r.copy()
            r["msg_index"] += off
            out_d.append(d)
            out_r.append(r)
        return np.concatenate(out_d), np.concatenate(out_r)

    def wait(self, timeout_ms: int = 1000) -> bool:
        """Park until a batch is in flight (True) or the timeout / a wake() passes (False)."""
        return self._L.rgb_wait(self._h, timeout_ms) == abi.OK

    def wake(self):
        self._L.rgb_wake(self._h)

    def submit_trains(self) -> int:
        """Batches whose sub-tick rounds ran as one train launch (rgb_submit_trains)."""
        return int(self._L.rgb_submit_trains(self._h))

    @property
    def in_flight(self) -> int:
        return int(self._L.rgb_in_flight(self._h))

    def step(self, msgs: np.ndarray, seq_ranges: np.ndarray | None = None):
        """submit + collect: decisions in submission order and the pipelined rpcs."""
        m = np.ascontiguousarray(msgs, dtype=abi.MSG_DTYPE)
        out_d, out_r = [], []
        for off in range(0, max(len(m), 1), self.ring_capacity):
            chunk = m[off:off + self.ring_capacity]
            self.submit(chunk, seq_ranges=seq_ranges)
            d, r, _ = self.collect(cap=max(len(chunk), 1))
            r = r.copy()
            r["msg_index"] += off
            out_d.append(d)
            out_r.append(r)
        return np.concatenate(out_d), np.concatenate(out_r)

    # -- device-resident path ------------------------------------------------------------
    def run_ticks_device(self, d_msgs: int, tick_stride: int, n_ticks: int, d_decisions: int,
                         d_rpcs: int = 0, stream: int = 0, tick_counts: np.ndarray | None = None,
                         d_tick_counts: int = 0, kind_counts: np.ndarray | None = None):
        """Raw device pointers (e.g. torch tensors' data_ptr()); enqueues and returns.
        tick_counts: messages per tick (uint32, host) or None for tick_stride each;
        d_tick_counts: device uint32 array with the real size of each tick (device producers);
        kind_counts: uint32 [n_ticks, n_kinds] (host) for family-ordered ticks -> specialised,
        concurrent per-kind kernels."""
        cp = None
        if tick_counts is not None:
            tc = np.ascontiguousarray(tick_counts, dtype=np.uint32)
            assert len(tc) >= n_ticks
            cp = tc.ctypes.data
        kp = None
        if kind_counts is not None:
            kcs = np.ascontiguousarray(kind_counts, dtype=np.uint32)
            assert kcs.shape == (n_ticks, abi.N_KINDS), kcs.shape
            kp = kcs.ctypes.data
        self._check(self._L.rgb_run_ticks_device(self._h, d_msgs, tick_stride, cp, d_tick_counts or None, kp,
                                                 n_ticks, d_decisions, d_rpcs or None, stream or None),
                    "rgb_run_ticks_device")

    def synth_tick_device(self, seed: int, tick: int, d_msgs: int, d_kind_counts: int = 0, d_n: int = 0,
                          stream: int = 0):
        """Device-side load generator (include/ra_gpu_batch_synth.h): one compacted, family-ordered
        tick from the current device state into d_msgs (room for n_servers messages)."""
        self._check(self._L.rgb_synth_tick_device(self._h, seed, tick, d_msgs, d_kind_counts or None,
                                                  d_n or None, stream or None), "rgb_synth_tick_device")

    def synth_tick_buckets_device(self, seed: int, tick: int, d_msgs: int, d_kind_counts: int = 0, d_n: int = 0,
                                  d_bucket_counts: int = 0, stream: int = 0):
        """The load generator, also writing uint32[TRAIN_BUCKETS] message counts per train bucket."""
        self._check(self._L.rgb_synth_tick_buckets_device(self._h, seed & (2**64 - 1), tick, d_msgs, d_kind_counts,
                                                         d_n, d_bucket_counts, stream), "rgb_synth_tick_buckets_device")

    def synth_tick_stamped_device(self, seed: int, tick: int, d_msgs: int, d_kind_counts: int = 0, d_n: int = 0,
                                  d_bucket_counts: int = 0, d_stamps: int = 0, stream: int = 0):
        """The load generator, also writing the tick's train stamps (uint8 per message slot): the producer's own
        count of the messages it has addressed to each server."""
        self._check(self._L.rgb_synth_tick_stamped_device(self._h, seed & (2**64 - 1), tick, d_msgs, d_kind_counts,
                                                         d_n, d_bucket_counts, d_stamps, stream),
                    "rgb_synth_tick_stamped_device")

    def synth_stamps_resync_device(self, stream: int = 0):
        """The generator's per-server message counts := the servers' sequence bytes as they are now."""
        self._check(self._L.rgb_synth_stamps_resync_device(self._h, stream), "rgb_synth_stamps_resync_device")

    # ---- train launches: several device-resident ticks in one launch ----
    def train_plan(self, bucket_counts: np.ndarray) -> "TrainPlan":
        return TrainPlan(self, bucket_counts)

    def train_stamp_device(self, d_msgs: int, d_stamps: int, tick_stride: int, tick_counts: np.ndarray, stream: int = 0):
        """d_stamps: uint8[n_ticks * tick_stride] on the device, the sequence value every message must find."""
        tc = np.ascontiguousarray(tick_counts, dtype=np.uint32)
        self._check(self._L.rgb_train_stamp_device(self._h, d_msgs, d_stamps, tick_stride, tc.ctypes.data, len(tc),
                                                   stream), "rgb_train_stamp_device")

    def train_run_device(self, plan: "TrainPlan", first_tick: int, n_ticks: int, d_msgs: int, d_stamps: int,
                         tick_stride: int, d_decisions: int, d_rpcs: int = 0, rpc_ring: int = 1, stream: int = 0):
        self._check(self._L.rgb_train_run_device(self._h, plan.h, first_tick, n_ticks, d_msgs, d_stamps, tick_stride,
                                                 d_decisions, d_rpcs, rpc_ring, stream), "rgb_train_run_device")

    def train_plan_snap(self, bucket_counts: np.ndarray, snapshot_every: int) -> "TrainPlan":
        """A plan whose ticks k * snapshot_every (k >= 1) carry the leaderboard snapshot in front of them."""
        return TrainPlan(self, bucket_counts, snapshot_every)

    def train_run_snap_device(self, plan: "TrainPlan", first_tick: int, n_ticks: int, d_msgs: int, d_stamps: int,
                              tick_stride: int, d_decisions: int, d_rpcs: int, rpc_ring: int, d_snap_stamps: int,
                              d_snap_rows: int, stream: int = 0):
        self._check(self._L.rgb_train_run_snap_device(self._h, plan.h, first_tick, n_ticks, d_msgs, d_stamps, tick_stride,
                                                      d_decisions, d_rpcs, rpc_ring, d_snap_stamps, d_snap_rows, stream),
                    "rgb_train_run_snap_device")

    def snapshot_train_device(self, d_rows: int, stream: int = 0):
        """rgb_snapshot_device + every sequence byte advanced (a snapshot boundary between two train launches)."""
        self._check(self._L.rgb_snapshot_train_device(self._h, d_rows, stream or None), "rgb_snapshot_train_device")

    def train_seq_bytes(self) -> int:
        return int(self._L.rgb_train_seq_bytes(self._h))

    def synth_snapshot_mark_device(self, d_snap_stamps: int = 0, stream: int = 0):
        """The generator's side of a snapshot boundary: its counts -> d_snap_stamps, then + 1."""
        self._check(self._L.rgb_synth_snapshot_mark_device(self._h, d_snap_stamps or None, stream or None),
                    "rgb_synth_snapshot_mark_device")

    def train_status(self, check: bool = True):
        """(error flags, XCD of every shard) of the trains run since the last call; the caller has synchronised."""
        flags = C.c_uint32(0)
        xcc = np.zeros(8, dtype=np.uint32)
        rc = self._L.rgb_train_status(self._h, C.byref(flags), xcc.ctypes.data)
        if check and rc:
            raise RgbError(rc, f"train launch failed (flags={flags.value}: 1 = placement, 2 = spin bound)")
        return int(flags.value), xcc

    def inject_train_fault(self, fault: int):
        """Fail-safe tests: the next train batch of submit() gets a fault (1 = a stamp that never comes up,
        2 = two messages bucketed under each other's shard).  The engine must repair the failed launch itself."""
        self._L.rgb_debug_inject_train_fault(self._h, fault)

    def train_form(self) -> str:
        return {0: "none", 1: "dealt", 2: "persistent"}[int(self._L.rgb_train_form(self._h))] if hasattr(self._L, "rgb_train_form") else "round-3 build"

    def train_recoveries(self) -> int:
        return int(self._L.rgb_train_recoveries(self._h))

    def synth_set_hint(self, level: int):
        """The generator's ordering hint (include/ra_gpu_batch_synth.h): 0 none, 1 state name, 2 + header compare."""
        self._check(self._L.rgb_synth_set_hint(self._h, level), "rgb_synth_set_hint")

    def synth_apply_tick_device(self, d_msgs: int, max_msgs: int, d_decisions: int, d_rpcs: int = 0,
                                stream: int = 0):
        """Apply the tick just generated by synth_tick_device (class-dispatch kernel sized on-device)."""
        self._check(self._L.rgb_synth_apply_tick_device(self._h, d_msgs, max_msgs, d_decisions, d_rpcs or None,
                                                        stream or None), "rgb_synth_apply_tick_device")

    # -- WAL entry checksums (include/ra_gpu_wal.h) -----------------------------------
    def wal_adler32_device(self, d_entries: int, n: int, d_data: int, data_bytes: int, d_checksums: int,
                           stream: int = 0):
        """adler32(<<Idx:64, Term:64, Payload>>) of n rgb_wal_entry records whose payloads are
        resident in device memory (src/ra_log_wal.erl:528-534, 861, 873, 1028); enqueues and returns."""
        self._check(self._L.rgb_wal_adler32_device(self._h, d_entries, n, d_data, data_bytes, d_checksums,
                                                   stream or None), "rgb_wal_adler32_device")

    def wal_adler32(self, entries: np.ndarray, data: np.ndarray) -> np.ndarray:
        """Host-buffer form: checksums of `entries` (abi.WAL_ENTRY_DTYPE) over the packed payload bytes."""
        entries = np.ascontiguousarray(entries, dtype=abi.WAL_ENTRY_DTYPE)
        data = np.ascontiguousarray(data, dtype=np.uint8)
        out = np.zeros(len(entries), dtype=np.uint32)
        self._check(self._L.rgb_wal_adler32(self._h, entries.ctypes.data, len(entries),
                                            data.ctypes.data if len(data) else None, len(data),
                                            out.ctypes.data), "rgb_wal_adler32")
        return out

    # -- WAL record framing and recovery validation (include/ra_gpu_wal.h) ---------------
    def wal_frame_device(self, d_records: int, n: int, d_data: int, data_bytes: int, d_out: int, out_bytes: int,
                         d_checksums: int = 0, flags: int = 0, stream: int = 0):
        """Frame n rgb_wal_record records into d_out (src/ra_log_wal.erl:513-537); enqueues and returns."""
        self._check(self._L.rgb_wal_frame_device(self._h, d_records, n, d_data, data_bytes, d_out, out_bytes,
                                                 d_checksums or None, flags, stream or None), "rgb_wal_frame_device")

    def wal_frame(self, records: np.ndarray, data: np.ndarray, out_bytes: int, flags: int = 0) -> np.ndarray:
        """Host-buffer form: the framed bytes [0, out_bytes) of `records` (abi.WAL_RECORD_DTYPE)."""
        records = np.ascontiguousarray(records, dtype=abi.WAL_RECORD_DTYPE)
        data = np.ascontiguousarray(data, dtype=np.uint8)
        out = np.zeros(out_bytes, dtype=np.uint8)
        self._check(self._L.rgb_wal_frame(self._h, records.ctypes.data, len(records),
                                          data.ctypes.data if len(data) else None, len(data),
                                          out.ctypes.data if out_bytes else None, out_bytes, flags), "rgb_wal_frame")
        return out

    def wal_validate(self, file_bytes: np.ndarray, scanned: np.ndarray):
        """(n_ok, status) of the scanned records of a WAL file: validate_checksum/4 on every record
        flagged WAL_REC_VALIDATE, is_last_record/3 on the first failure (src/ra_log_wal.erl:994-1033)."""
        file_bytes = np.ascontiguousarray(file_bytes, dtype=np.uint8)
        scanned = np.ascontiguousarray(scanned, dtype=abi.WAL_SCANNED_DTYPE)
        n_ok, status = C.c_uint32(0), C.c_uint32(0)
        self._check(self._L.rgb_wal_validate(self._h, file_bytes.ctypes.data, len(file_bytes),
                                             scanned.ctypes.data if len(scanned) else None, len(scanned),
                                             C.byref(n_ok), C.byref(status)), "rgb_wal_validate")
        return n_ok.value, status.value

    # -- WAL batch: a mailbox-ordered batch of append commands in one call (include/ra_gpu_wal.h) --
    def wal_batch_device(self, cmds: np.ndarray, writers: np.ndarray, file: np.ndarray, d_data: int, data_bytes: int,
                         d_results: int, d_writers_out: int, d_out: int, out_bytes: int, d_events: int, events_cap: int,
                         d_ranges: int, ranges_cap: int, d_total: int, flags: int = 0, stream: int = 0):
        """ra_log_wal:handle_batch/2 for a batch of append commands (src/ra_log_wal.erl:482-635, 800-812, 1050-1066):
        abi.WAL_CMD_RESULT_DTYPE rows, the new abi.WAL_WRITER_DTYPE rows, the framed bytes, abi.WAL_EVENT_DTYPE rows
        with their (first, last) pairs and one abi.WAL_BATCH_TOTAL_DTYPE record, all into device memory.  `cmds`,
        `writers` and `file` are host arrays; enqueues and returns."""
        cmds = np.ascontiguousarray(cmds, dtype=abi.WAL_CMD_DTYPE)
        writers = np.ascontiguousarray(writers, dtype=abi.WAL_WRITER_DTYPE)
        file = np.ascontiguousarray(file, dtype=abi.WAL_FILE_DTYPE).reshape(1)
        self._check(self._L.rgb_wal_batch_device(self._h, cmds.ctypes.data if len(cmds) else None, len(cmds),
                                                 writers.ctypes.data if len(writers) else None, len(writers),
                                                 file.ctypes.data, d_data or None, data_bytes, flags, d_results or None,
                                                 d_writers_out or None, d_out or None, out_bytes, d_events or None,
                                                 events_cap, d_ranges or None, ranges_cap, d_total or None,
                                                 stream or None), "rgb_wal_batch_device")

    def wal_batch(self, cmds: np.ndarray, writers: np.ndarray, file: np.ndarray, data: np.ndarray, flags: int = 0,
                  out_bytes: int | None = None, events_cap: int | None = None, ranges_cap: int | None = None):
        """Host-buffer form: (total record, result rows, writer rows, out bytes, event rows, pairs as an (n_ranges, 2)
        array).  The buffers default to wal_batch_bound's sizes.  With abi.WAL_BATCH_SPACE the out bytes are None,
        and events and pairs are None unless both fit their caps."""
        cmds = np.ascontiguousarray(cmds, dtype=abi.WAL_CMD_DTYPE)
        writers = np.ascontiguousarray(writers, dtype=abi.WAL_WRITER_DTYPE)
        file = np.ascontiguousarray(file, dtype=abi.WAL_FILE_DTYPE).reshape(1)
        data = np.ascontiguousarray(data, dtype=np.uint8)
        if out_bytes is None or events_cap is None or ranges_cap is None:
            ob, eb, rb = wal_batch_bound(cmds, writers, file, len(data))
            out_bytes = ob if out_bytes is None else out_bytes
            events_cap = eb if events_cap is None else events_cap
            ranges_cap = rb if ranges_cap is None else ranges_cap
        results = np.zeros(len(cmds), dtype=abi.WAL_CMD_RESULT_DTYPE)
        writers_out = np.zeros(len(writers), dtype=abi.WAL_WRITER_DTYPE)
        out = np.zeros(out_bytes, dtype=np.uint8)
        events = np.zeros(events_cap, dtype=abi.WAL_EVENT_DTYPE)
        ranges = np.zeros((ranges_cap, 2), dtype=np.uint64)
        total = np.zeros(1, dtype=abi.WAL_BATCH_TOTAL_DTYPE)
        self._check(self._L.rgb_wal_batch(self._h, cmds.ctypes.data if len(cmds) else None, len(cmds),
                                          writers.ctypes.data if len(writers) else None, len(writers), file.ctypes.data,
                                          data.ctypes.data if len(data) else None, len(data), flags,
                                          results.ctypes.data if len(cmds) else None,
                                          writers_out.ctypes.data if len(writers) else None,
                                          out.ctypes.data if out_bytes else None, out_bytes,
                                          events.ctypes.data if events_cap else None, events_cap,
                                          ranges.ctypes.data if ranges_cap else None, ranges_cap, total.ctypes.data),
                    "rgb_wal_batch")
        t = total[0]
        fit = int(t["n_events"]) <= events_cap and int(t["n_ranges"]) <= ranges_cap
        space = int(t["status"]) == abi.WAL_BATCH_SPACE
        return (t, results, writers_out, None if space else out[:int(t["out_bytes"])],
                events[:int(t["n_events"])] if fit else None, ranges[:int(t["n_ranges"])] if fit else None)

    # -- segments and snapshots: batched CRC-32 (include/ra_gpu_wal.h) ------------------
    def crc32_device(self, d_entries: int, n: int, d_data: int, data_bytes: int, d_crcs: int, stream: int = 0):
        """erlang:crc32(Payload) of n rgb_seg_entry records whose payloads are resident in device memory
        (src/ra_log_segment.erl:277, 670, 1240-1248); enqueues and returns."""
        self._check(self._L.rgb_crc32_device(self._h, d_entries, n, d_data, data_bytes, d_crcs, stream or None),
                    "rgb_crc32_device")

    def crc32(self, entries: np.ndarray, data: np.ndarray) -> np.ndarray:
        """Host-buffer form: CRC-32 of `entries` (abi.SEG_ENTRY_DTYPE) over the packed payload bytes."""
        entries = np.ascontiguousarray(entries, dtype=abi.SEG_ENTRY_DTYPE)
        data = np.ascontiguousarray(data, dtype=np.uint8)
        out = np.zeros(len(entries), dtype=np.uint32)
        self._check(self._L.rgb_crc32(self._h, entries.ctypes.data, len(entries),
                                      data.ctypes.data if len(data) else None, len(data), out.ctypes.data), "rgb_crc32")
        return out

    def crc32_stream_device(self, d_data: int, n_bytes: int, init: int, d_crc: int, stream: int = 0):
        """*d_crc = erlang:crc32(init, Data) of one long device buffer (src/ra_log_snapshot.erl:57-107); enqueues."""
        self._check(self._L.rgb_crc32_stream_device(self._h, d_data or None, n_bytes, init, d_crc, stream or None),
                    "rgb_crc32_stream_device")

    def crc32_stream(self, data, init: int = 0) -> int:
        """Host-buffer form of crc32_stream_device: zlib.crc32(data, init)."""
        data = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else \
            np.ascontiguousarray(data, dtype=np.uint8)
        out = C.c_uint32(0)
        self._check(self._L.rgb_crc32_stream(self._h, data.ctypes.data if len(data) else None, len(data), init,
                                             C.byref(out)), "rgb_crc32_stream")
        return out.value

    def segment_build_device(self, d_entries: int, n: int, max_count: int, d_out_offsets: int, d_data: int,
                             data_bytes: int, d_out: int, out_bytes: int, flags: int = 0, stream: int = 0):
        """The whole segment file image of n entries into d_out (src/ra_log_segment.erl:1118-1122, 1211-1219):
        header, index records, zeros for the unused records, payload copies; enqueues and returns."""
        self._check(self._L.rgb_segment_build_device(self._h, d_entries or None, n, max_count, d_out_offsets or None,
                                                     d_data or None, data_bytes, d_out, out_bytes, flags,
                                                     stream or None), "rgb_segment_build_device")

    def segment_build(self, entries: np.ndarray, data: np.ndarray, max_count: int = 4096, flags: int = 0,
                      out: np.ndarray | None = None) -> np.ndarray:
        """Host-buffer form: the file bytes of `entries` (abi.SEG_ENTRY_DTYPE).  `out` (uint8, at least the file
        size) is filled in place when given; bytes behind the file size are left alone."""
        entries = np.ascontiguousarray(entries, dtype=abi.SEG_ENTRY_DTYPE)
        data = np.ascontiguousarray(data, dtype=np.uint8)
        if out is None:
            out = np.zeros(segment_layout(entries, max_count)[1], dtype=np.uint8)
        self._check(self._L.rgb_segment_build(self._h, entries.ctypes.data if len(entries) else None, len(entries),
                                              max_count, data.ctypes.data if len(data) else None, len(data),
                                              out.ctypes.data, len(out), flags), "rgb_segment_build")
        return out

    def segment_validate(self, file_bytes: np.ndarray, recs: np.ndarray) -> int:
        """Number of leading records of a scanned segment whose payload matches the stored CRC (0 = not checked,
        src/ra_log_segment.erl:1245-1248)."""
        file_bytes = np.ascontiguousarray(file_bytes, dtype=np.uint8)
        recs = np.ascontiguousarray(recs, dtype=abi.SEG_ENTRY_DTYPE)
        n_ok = C.c_uint32(0)
        self._check(self._L.rgb_segment_validate(self._h, file_bytes.ctypes.data if len(file_bytes) else None,
                                                 len(file_bytes), recs.ctypes.data if len(recs) else None, len(recs),
                                                 C.byref(n_ok)), "rgb_segment_validate")
        return n_ok.value

    # -- major compaction: info/2 and copy/3 of a group of segment files (include/ra_gpu_wal.h) --
    def segment_info_device(self, sources: np.ndarray, d_files: int, files_bytes: int, live, d_infos: int,
                            stream: int = 0):
        """One abi.SEG_INFO_DTYPE row per source into d_infos (ra_log_segment:info/2, src/ra_log_segment.erl:736-790).
        `sources` (abi.SEG_SOURCE_DTYPE) and `live` ((first, last) pairs of uint64, or None: every record counts into
        live_size) are host arrays; enqueues and returns."""
        sources, live, n_live = _compact_args(sources, live)
        self._check(self._L.rgb_segment_info_device(self._h, sources.ctypes.data if len(sources) else None, len(sources),
                                                    d_files or None, files_bytes,
                                                    live.ctypes.data if live is not None else None, n_live,
                                                    d_infos or None, stream or None), "rgb_segment_info_device")

    def segment_info(self, sources: np.ndarray, files: np.ndarray, live=None) -> np.ndarray:
        """Host-buffer form of segment_info_device: the rows as abi.SEG_INFO_DTYPE."""
        sources, live, n_live = _compact_args(sources, live)
        files = np.ascontiguousarray(files, dtype=np.uint8)
        infos = np.zeros(len(sources), dtype=abi.SEG_INFO_DTYPE)
        self._check(self._L.rgb_segment_info(self._h, sources.ctypes.data if len(sources) else None, len(sources),
                                             files.ctypes.data if len(files) else None, len(files),
                                             live.ctypes.data if live is not None else None, n_live,
                                             infos.ctypes.data if len(sources) else None), "rgb_segment_info")
        return infos

    def segment_compact_device(self, sources: np.ndarray, d_files: int, files_bytes: int, live, d_out: int,
                               out_bytes: int, d_result: int, max_size: int = abi.SEG_MAX_SIZE_B, flags: int = 0,
                               stream: int = 0):
        """The live entries of every source copied into one new segment image at d_out (ra_log_segment:copy/3 for a
        compaction group, src/ra_log_segments.erl:741-835); *d_result = one abi.SEG_COMPACT_RESULT_DTYPE record.
        `sources` and `live` are host arrays; enqueues and returns."""
        sources, live, n_live = _compact_args(sources, live)
        self._check(self._L.rgb_segment_compact_device(self._h, sources.ctypes.data if len(sources) else None,
                                                       len(sources), d_files or None, files_bytes,
                                                       live.ctypes.data if live is not None else None, n_live, max_size,
                                                       flags, d_out or None, out_bytes, d_result or None,
                                                       stream or None), "rgb_segment_compact_device")

    def segment_compact(self, sources: np.ndarray, files: np.ndarray, live, max_size: int = abi.SEG_MAX_SIZE_B,
                        flags: int = 0, out: np.ndarray | None = None):
        """Host-buffer form: (result record, image).  The image is `out[:file_bytes]` when the status is
        abi.SEG_COMPACT_OK and None otherwise; `out` (uint8) defaults to a buffer of segment_compact_bound's size and is
        written only when the status is OK, and only its first file_bytes bytes."""
        sources, live, n_live = _compact_args(sources, live)
        files = np.ascontiguousarray(files, dtype=np.uint8)
        if out is None:
            out = np.zeros(segment_compact_bound(sources, live, len(files))[0], dtype=np.uint8)
        res = np.zeros(1, dtype=abi.SEG_COMPACT_RESULT_DTYPE)
        self._check(self._L.rgb_segment_compact(self._h, sources.ctypes.data if len(sources) else None, len(sources),
                                                files.ctypes.data if len(files) else None, len(files),
                                                live.ctypes.data if live is not None else None, n_live, max_size, flags,
                                                out.ctypes.data if len(out) else None, len(out), res.ctypes.data),
                    "rgb_segment_compact")
        ok = int(res["status"][0]) == abi.SEG_COMPACT_OK
        return res[0], (out[:int(res["file_bytes"][0])] if ok else None)

    # -- major compaction for many members: any number of groups in one call (include/ra_gpu_wal.h) --
    def segment_compact_groups_device(self, groups: np.ndarray, sources: np.ndarray, d_files: int, files_bytes: int, live,
                                      d_out: int, out_bytes: int, d_results: int, max_size: int = abi.SEG_MAX_SIZE_B,
                                      flags: int = 0, stream: int = 0):
        """Every group's image at d_out + out_offset and one abi.SEG_COMPACT_RESULT_DTYPE row per group into d_results:
        per group exactly what segment_compact_device gives for it alone.  `groups` (abi.SEG_GROUP_DTYPE), `sources` and
        `live` are host arrays; enqueues and returns."""
        groups = np.ascontiguousarray(groups, dtype=abi.SEG_GROUP_DTYPE)
        sources, live, n_live = _compact_args(sources, live)
        self._check(self._L.rgb_segment_compact_groups_device(
            self._h, groups.ctypes.data if len(groups) else None, len(groups),
            sources.ctypes.data if len(sources) else None, len(sources), d_files or None, files_bytes,
            live.ctypes.data if live is not None else None, n_live, max_size, flags, d_out or None, out_bytes,
            d_results or None, stream or None), "rgb_segment_compact_groups_device")

    def segment_compact_groups(self, groups: np.ndarray, sources: np.ndarray, files: np.ndarray, live,
                               max_size: int = abi.SEG_MAX_SIZE_B, flags: int = 0, out: np.ndarray | None = None):
        """Host-buffer form: (result rows, images).  images[g] is a view of `out` when the group's status is
        abi.SEG_COMPACT_OK and None otherwise; `out` (uint8) defaults to a buffer that ends with the last group's range,
        and only the good images' own bytes are written."""
        groups = np.ascontiguousarray(groups, dtype=abi.SEG_GROUP_DTYPE)
        sources, live, n_live = _compact_args(sources, live)
        files = np.ascontiguousarray(files, dtype=np.uint8)
        if out is None:
            out = np.zeros(max([int(g["out_offset"]) + int(g["out_bytes"]) for g in groups], default=0), dtype=np.uint8)
        res = np.zeros(len(groups), dtype=abi.SEG_COMPACT_RESULT_DTYPE)
        self._check(self._L.rgb_segment_compact_groups(
            self._h, groups.ctypes.data if len(groups) else None, len(groups),
            sources.ctypes.data if len(sources) else None, len(sources), files.ctypes.data if len(files) else None,
            len(files), live.ctypes.data if live is not None else None, n_live, max_size, flags,
            out.ctypes.data if len(out) else None, len(out), res.ctypes.data if len(groups) else None),
            "rgb_segment_compact_groups")
        images = [out[int(g["out_offset"]):int(g["out_offset"]) + int(r["file_bytes"])]
                  if int(r["status"]) == abi.SEG_COMPACT_OK else None for g, r in zip(groups, res)]
        return res, images

    def major_compaction_plan(self, members, files: np.ndarray, max_count: int = abi.SEG_MAX_ENTRIES,
                              max_size: int = abi.SEG_MAX_SIZE_B) -> dict:
        """The plan of ra_log_segments:major_compaction/3 (src/ra_log_segments.erl:741-835) for many members: select,
        then info/2 of every file that holds live indexes (in chunks of at most abi.SEG_COMPACT_MAX_SOURCES sources),
        then the groups.  `members`: per member (segrefs, live) -- segrefs a list of (offset, n_bytes, (range_first,
        range_last)) of the member's files inside `files`, newest first as compactable_segrefs/2 gives them; live the
        member's live pairs.  -> dict: `groups` (abi.SEG_GROUP_DTYPE, laid out back to back by
        segment_compact_groups_bound), `sources` (abi.SEG_SOURCE_DTYPE, the groups' sources oldest first), `live`
        (pairs), `out_bytes`, `max_counts`, and per member `group_files` (per group of `groups`, in order: (member,
        the file ordinals in the member's segref list)), `unreferenced` (file ordinals, the Delete list in the fold's
        order), `skipped` (compactable candidates that joined no group) and `status` (abi.SEG_TAKE_*); for callers
        that want to look further, `candidates` ((member, file ordinal, segref number) of every file with live indexes,
        oldest first per member) and their `infos` rows.
        info/2 goes through the host-buffer segment_info, which stages `files` once per chunk and answers a file
        with a damaged header with RgbError(RGB_E_INVAL) for the whole call -- as the reference's info/2 crashes the
        compaction that meets it: ONE such file among the candidates fails the plan of every member of the call,
        unlike the copy, where it fails its own group only.  A caller that must survive it plans such members apart."""
        files = np.ascontiguousarray(files, dtype=np.uint8)
        mem = np.zeros(len(members), dtype=abi.SEG_MEMBER_DTYPE)
        segrefs, live = [], []
        for m, (refs, pairs) in enumerate(members):
            pairs = np.asarray(pairs if pairs is not None else [], dtype=np.uint64).reshape(-1, 2)
            mem[m] = (len(segrefs), len(refs), len(live), len(pairs))
            segrefs += [(r[2][0], r[2][1]) for r in refs]
            live += [tuple(p) for p in pairs.tolist()]
        picks, live_out = segment_compact_select(mem, segrefs, live)
        # the candidates of every member, OLDEST first (the fold prepends): info/2 with the selection as the live list
        cand = np.zeros(len(picks), dtype=abi.SEG_SOURCE_DTYPE)
        where, take = [], np.zeros(len(members), dtype=abi.SEG_TAKE_MEMBER_DTYPE)
        unreferenced = [[] for _ in members]
        for m, (refs, _) in enumerate(members):
            first = len(where)
            base = int(mem["segref_first"][m])
            for k in range(len(refs)):
                if int(picks["flags"][base + k]) & abi.SEG_PICK_UNREFERENCED:
                    unreferenced[m].insert(0, k)                      # [Fn0 | Del]
            for k in reversed(range(len(refs))):
                if not int(picks["flags"][base + k]) & abi.SEG_PICK_UNREFERENCED:
                    cand[len(where)] = (refs[k][0], refs[k][1], picks["live_first"][base + k], picks["live_n"][base + k], 0)
                    where.append((m, k, base + k))
            take[m] = (first, len(where) - first, 0, 0)
        cand = cand[:len(where)]
        infos = np.zeros(len(cand), dtype=abi.SEG_INFO_DTYPE)
        for lo in range(0, len(cand), abi.SEG_COMPACT_MAX_SOURCES):
            hi = min(len(cand), lo + abi.SEG_COMPACT_MAX_SOURCES)
            infos[lo:hi] = self.segment_info(cand[lo:hi], files, live_out)
        num_live = np.array([int(picks["num_live"][w[2]]) for w in where], dtype=np.uint64)
        take, group_of = segment_compact_take_groups(take, infos, num_live, max_count, max_size)
        rows, sources, group_files, skipped = [], [], [], [[] for _ in members]
        for m in range(len(members)):
            first, n = int(take["src_first"][m]), int(take["src_n"][m])
            for g in range(int(take["n_groups"][m])):
                idx = [first + j for j in range(n) if int(group_of[first + j]) == g]
                rows.append((len(sources), len(idx), 0, 0))
                sources += idx
                group_files.append((m, [where[i][1] for i in idx]))
            skipped[m] = [where[first + j][1] for j in range(n) if int(group_of[first + j]) == abi.SEG_GROUP_NONE]
        groups = np.array(rows, dtype=abi.SEG_GROUP_DTYPE).reshape(-1)
        sources = cand[np.array(sources, dtype=np.int64)]
        groups, out_bytes, max_counts = segment_compact_groups_bound(groups, sources, live_out, len(files))
        return dict(groups=groups, sources=sources, live=live_out, out_bytes=out_bytes, max_counts=max_counts,
                    group_files=group_files, unreferenced=unreferenced, skipped=skipped,
                    status=[int(x) for x in take["status"]], infos=infos, candidates=where)

    # -- mem-table flush: the entries of many writers into their segment files (include/ra_gpu_wal.h) --
    def segment_flush_device(self, writers: np.ndarray, d_entries: int, n_entries: int, d_data: int, data_bytes: int,
                             d_pieces: int, pieces_cap: int, d_out: int, out_bytes: int, d_result: int,
                             max_count: int = abi.SEG_MAX_ENTRIES, max_size: int = abi.SEG_MAX_SIZE_B, flags: int = 0,
                             stream: int = 0):
        """The entries of every writer split over its open segment and successors (ra_log_segment_writer's flush,
        src/ra_log_segment_writer.erl:268-329, 425-500): abi.SEG_PIECE_DTYPE rows into d_pieces, the bytes to pwrite
        into d_out, one abi.SEG_FLUSH_RESULT_DTYPE record into d_result.  `writers` (abi.SEG_WRITER_DTYPE) is a host
        array; enqueues and returns."""
        writers = np.ascontiguousarray(writers, dtype=abi.SEG_WRITER_DTYPE)
        self._check(self._L.rgb_segment_flush_device(self._h, writers.ctypes.data if len(writers) else None, len(writers),
                                                     d_entries or None, n_entries, d_data or None, data_bytes, max_count,
                                                     max_size, flags, d_pieces or None, pieces_cap, d_out or None,
                                                     out_bytes, d_result or None, stream or None),
                    "rgb_segment_flush_device")

    def segment_flush(self, writers: np.ndarray, entries: np.ndarray, data: np.ndarray,
                      max_count: int = abi.SEG_MAX_ENTRIES, max_size: int = abi.SEG_MAX_SIZE_B, flags: int = 0,
                      pieces: np.ndarray | None = None, out: np.ndarray | None = None):
        """Host-buffer form: (result record, piece rows, out bytes).  Rows and bytes are `pieces[:n_pieces]` and
        `out[:out_bytes]` when the status is abi.SEG_FLUSH_OK and None otherwise; both buffers default to
        segment_flush_bound's sizes and are written only when the status is OK."""
        writers = np.ascontiguousarray(writers, dtype=abi.SEG_WRITER_DTYPE)
        entries = np.ascontiguousarray(entries, dtype=abi.SEG_ENTRY_DTYPE)
        data = np.ascontiguousarray(data, dtype=np.uint8)
        if pieces is None or out is None:
            out_bound, pieces_bound = segment_flush_bound(writers, len(entries), len(data))
            pieces = np.zeros(pieces_bound, dtype=abi.SEG_PIECE_DTYPE) if pieces is None else pieces
            out = np.zeros(out_bound, dtype=np.uint8) if out is None else out
        res = np.zeros(1, dtype=abi.SEG_FLUSH_RESULT_DTYPE)
        self._check(self._L.rgb_segment_flush(self._h, writers.ctypes.data if len(writers) else None, len(writers),
                                              entries.ctypes.data if len(entries) else None, len(entries),
                                              data.ctypes.data if len(data) else None, len(data), max_count, max_size,
                                              flags, pieces.ctypes.data if len(pieces) else None, len(pieces),
                                              out.ctypes.data if len(out) else None, len(out), res.ctypes.data),
                    "rgb_segment_flush")
        if int(res["status"][0]) != abi.SEG_FLUSH_OK:
            return res[0], None, None
        return res[0], pieces[:int(res["n_pieces"][0])], out[:int(res["out_bytes"][0])]

    # -- reading entries back: read plans, folds and term queries over many segment files (include/ra_gpu_wal.h) --
    def segment_read_device(self, sources: np.ndarray, d_files: int, files_bytes: int, req, d_rows: int, d_out: int,
                            out_bytes: int, d_results: int, d_total: int, flags: int = 0, stream: int = 0):
        """One abi.SEG_ENTRY_DTYPE row per requested index into d_rows, the payloads back to back in request order into
        d_out, one abi.SEG_READ_RESULT_DTYPE row per source into d_results, one abi.SEG_READ_TOTAL_DTYPE record into
        d_total (ra_log_segment:read_sparse/4, fold/6 and term_query/2 over many files).  `sources`
        (abi.SEG_READ_SOURCE_DTYPE) and `req` (uint64 indexes) are host arrays; enqueues and returns."""
        sources = np.ascontiguousarray(sources, dtype=abi.SEG_READ_SOURCE_DTYPE)
        req = np.ascontiguousarray(req, dtype=np.uint64)
        self._check(self._L.rgb_segment_read_device(self._h, sources.ctypes.data if len(sources) else None, len(sources),
                                                    d_files or None, files_bytes, req.ctypes.data if len(req) else None,
                                                    len(req), flags, d_rows or None, d_out or None, out_bytes,
                                                    d_results or None, d_total or None, stream or None),
                    "rgb_segment_read_device")

    def segment_read(self, sources: np.ndarray, files: np.ndarray, req, flags: int = 0, rows: np.ndarray | None = None,
                     out: np.ndarray | None = None):
        """Host-buffer form: (total record, result rows, rows, out bytes).  `rows` (abi.SEG_ENTRY_DTYPE, one per
        request; only those a slice names are written) defaults to a zeroed array.  Without `out` the call sizes it
        itself (a sizing call first, unless abi.SEG_READ_NO_DATA is set); with `out` the bytes are `out[:out_bytes]`
        when the total's status is abi.SEG_READ_OK and None when it is abi.SEG_READ_SPACE."""
        sources = np.ascontiguousarray(sources, dtype=abi.SEG_READ_SOURCE_DTYPE)
        files = np.ascontiguousarray(files, dtype=np.uint8)
        req = np.ascontiguousarray(req, dtype=np.uint64)
        if rows is None:
            rows = np.zeros(len(req), dtype=abi.SEG_ENTRY_DTYPE)
        results = np.zeros(len(sources), dtype=abi.SEG_READ_RESULT_DTYPE)
        total = np.zeros(1, dtype=abi.SEG_READ_TOTAL_DTYPE)

        def call(buf):
            self._check(self._L.rgb_segment_read(self._h, sources.ctypes.data if len(sources) else None, len(sources),
                                                 files.ctypes.data if len(files) else None, len(files),
                                                 req.ctypes.data if len(req) else None, len(req), flags,
                                                 rows.ctypes.data if len(rows) else None,
                                                 buf.ctypes.data if buf is not None and len(buf) else None,
                                                 0 if buf is None else len(buf), results.ctypes.data if len(sources) else None,
                                                 total.ctypes.data), "rgb_segment_read")
        call(out)
        if out is None and int(total["status"][0]) == abi.SEG_READ_SPACE:
            out = np.zeros(int(total["out_bytes"][0]), dtype=np.uint8)
            call(out)
        if int(total["status"][0]) != abi.SEG_READ_OK:
            return total[0], results, rows, None
        return total[0], results, rows, (out[:int(total["out_bytes"][0])] if out is not None else np.zeros(0, dtype=np.uint8))

    # -- snapshots and checkpoints: ragged CRC batches, images, validation (include/ra_gpu_wal.h) --
    def crc32_spans_device(self, spans: np.ndarray, d_data: int, data_bytes: int, d_crcs: int, stream: int = 0):
        """d_crcs[i] = erlang:crc32(init_i, span i) for `spans` (abi.CRC_SPAN_DTYPE, a host array) over a device
        buffer: accept_chunk/2 of every transfer in flight (src/ra_log_snapshot.erl:104-108); enqueues and returns."""
        spans = np.ascontiguousarray(spans, dtype=abi.CRC_SPAN_DTYPE)
        self._check(self._L.rgb_crc32_spans_device(self._h, spans.ctypes.data if len(spans) else None, len(spans),
                                                   d_data or None, data_bytes, d_crcs or None, stream or None),
                    "rgb_crc32_spans_device")

    def crc32_spans(self, spans: np.ndarray, data) -> np.ndarray:
        """Host-buffer form of crc32_spans_device: zlib.crc32(span, init) per span."""
        spans = np.ascontiguousarray(spans, dtype=abi.CRC_SPAN_DTYPE)
        data = np.ascontiguousarray(data, dtype=np.uint8)
        out = np.zeros(len(spans), dtype=np.uint32)
        self._check(self._L.rgb_crc32_spans(self._h, spans.ctypes.data if len(spans) else None, len(spans),
                                            data.ctypes.data if len(data) else None, len(data),
                                            out.ctypes.data if len(spans) else None), "rgb_crc32_spans")
        return out

    def snapshot_build_device(self, items: np.ndarray, d_data: int, data_bytes: int, d_out: int, out_bytes: int,
                              d_crcs: int = 0, stream: int = 0):
        """The snapshot.dat / indexes image of every item (abi.SNAP_ITEM_DTYPE, a host array, out_offset filled) into
        d_out (src/ra_log_snapshot.erl:49-68, src/ra_snapshot.erl:1017-1026); enqueues and returns."""
        items = np.ascontiguousarray(items, dtype=abi.SNAP_ITEM_DTYPE)
        self._check(self._L.rgb_snapshot_build_device(self._h, items.ctypes.data if len(items) else None, len(items),
                                                      d_data or None, data_bytes, d_out or None, out_bytes,
                                                      d_crcs or None, stream or None), "rgb_snapshot_build_device")

    def snapshot_build(self, items: np.ndarray, data, out: np.ndarray | None = None):
        """Host-buffer form: (image bytes, the Crc of every image).  Without `out` the items are laid out back to
        back from 0 (their out_offset is overwritten in a copy); with `out` they go where their out_offset says."""
        items = np.ascontiguousarray(items, dtype=abi.SNAP_ITEM_DTYPE)
        data = np.ascontiguousarray(data, dtype=np.uint8)
        if out is None:
            items, size = snapshot_layout(items)
            out = np.zeros(size, dtype=np.uint8)
        crcs = np.zeros(len(items), dtype=np.uint32)
        self._check(self._L.rgb_snapshot_build(self._h, items.ctypes.data if len(items) else None, len(items),
                                               data.ctypes.data if len(data) else None, len(data),
                                               out.ctypes.data if len(out) else None, len(out),
                                               crcs.ctypes.data if len(items) else None), "rgb_snapshot_build")
        return out, crcs

    def snapshot_validate_device(self, files: np.ndarray, d_files: int, files_bytes: int, d_infos: int, stream: int = 0):
        """One abi.SNAP_INFO_DTYPE row per file of `files` (abi.SNAP_FILE_DTYPE, a host array) into d_infos:
        recover/1, validate/1 and read_meta/1 (src/ra_log_snapshot.erl:176-266); enqueues and returns."""
        files = np.ascontiguousarray(files, dtype=abi.SNAP_FILE_DTYPE)
        self._check(self._L.rgb_snapshot_validate_device(self._h, files.ctypes.data if len(files) else None, len(files),
                                                         d_files or None, files_bytes, d_infos or None, stream or None),
                    "rgb_snapshot_validate_device")

    def snapshot_validate(self, files: np.ndarray, file_bytes) -> np.ndarray:
        """Host-buffer form of snapshot_validate_device: the info rows."""
        files = np.ascontiguousarray(files, dtype=abi.SNAP_FILE_DTYPE)
        file_bytes = np.ascontiguousarray(file_bytes, dtype=np.uint8)
        infos = np.zeros(len(files), dtype=abi.SNAP_INFO_DTYPE)
        self._check(self._L.rgb_snapshot_validate(self._h, files.ctypes.data if len(files) else None, len(files),
                                                  file_bytes.ctypes.data if len(file_bytes) else None, len(file_bytes),
                                                  infos.ctypes.data if len(files) else None), "rgb_snapshot_validate")
        return infos

    # -- observability -----------------------------------------------------------------
    def snapshot(self) -> np.ndarray:
        rows = np.zeros(self.n_groups, dtype=abi.LEADERBOARD_DTYPE)
        self._check(self._L.rgb_snapshot(self._h, rows.ctypes.data), "rgb_snapshot")
        return rows

    def snapshot_device(self, d_rows: int, stream: int = 0):
        self._check(self._L.rgb_snapshot_device(self._h, d_rows, stream or None), "rgb_snapshot_device")

    def state_checksum(self, first: int = 0, n: int | None = None) -> int:
        n = self.n_servers - first if n is None else n
        out = C.c_uint64(0)
        self._check(self._L.rgb_state_checksum(self._h, first, n, C.byref(out)), "rgb_state_checksum")
        return out.value

    def synchronize(self):
        self._check(self._L.rgb_synchronize(self._h), "rgb_synchronize")


TRAIN_BUCKETS = 256


def comm_unique_id() -> bytes:
    """RGB_COMM_ID_BYTES of a fresh communicator id (one rank creates it, the others receive it from the host)."""
    buf = C.create_string_buffer(abi.COMM_ID_BYTES)
    rc = lib().rgb_comm_unique_id(buf)
    if rc:
        raise RgbError(rc, "rgb_comm_unique_id")
    return buf.raw


class Comm:
    """rgb_comm: this context's rank in the leaderboard all-gather (RCCL behind the C ABI)."""

    def __init__(self, eng: "RaGpuBatch", comm_id: bytes, n_ranks: int, rank: int):
        assert len(comm_id) == abi.COMM_ID_BYTES
        self.eng, self.n_ranks, self.rank = eng, n_ranks, rank
        h = C.c_void_p()
        rc = eng._L.rgb_comm_init_rank(eng._h, comm_id, n_ranks, rank, C.byref(h))
        if rc:
            raise RgbError(rc, f"rgb_comm_init_rank: {eng._L.rgb_comm_last_error().decode()}")
        self.h = h

    def allgather_leaderboard(self, d_rows_local: int, n_rows: int, d_rows_all: int, stream: int = 0):
        """Every rank's n_rows leaderboard rows (device memory) -> d_rows_all[rank * n_rows ..], on `stream`."""
        rc = self.eng._L.rgb_leaderboard_allgather(self.eng._h, self.h, d_rows_local, n_rows, d_rows_all, stream or None)
        if rc:
            raise RgbError(rc, f"rgb_leaderboard_allgather: {self.eng._L.rgb_comm_last_error().decode()}")

    def close(self):
        if self.h:
            self.eng._L.rgb_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TrainPlan:
    """Device plan of a train (rgb_train_plan): bucket_counts = uint32[n_ticks][TRAIN_BUCKETS]."""

    def __init__(self, eng: "RaGpuBatch", bucket_counts, snapshot_every: int = 0, device_ticks: int = 0):
        """bucket_counts (host array): the plan is built on the host and uploaded.  device_ticks > 0 (bucket_counts =
        None): an empty plan of that many ticks for build_device() -- rgb_train_plan_create_device."""
        h = C.c_void_p()
        if device_ticks:
            self.eng, self.n_ticks, self.snapshot_every = eng, device_ticks, snapshot_every
            eng._check(eng._L.rgb_train_plan_create_device(eng._h, device_ticks, snapshot_every, C.byref(h)),
                       "rgb_train_plan_create_device")
            self.h = h
            self.blocks_per_tick = int(eng._L.rgb_train_plan_blocks_per_tick(h))
            return
        bc = np.ascontiguousarray(bucket_counts, dtype=np.uint32).reshape(-1, TRAIN_BUCKETS)
        self.eng, self.n_ticks, self.snapshot_every = eng, len(bc), snapshot_every
        if snapshot_every:
            eng._check(eng._L.rgb_train_plan_create_snap(eng._h, bc.ctypes.data, len(bc), snapshot_every, C.byref(h)),
                       "rgb_train_plan_create_snap")
        else:
            eng._check(eng._L.rgb_train_plan_create(eng._h, bc.ctypes.data, len(bc), C.byref(h)), "rgb_train_plan_create")
        self.h = h
        self.blocks_per_tick = int(eng._L.rgb_train_plan_blocks_per_tick(h))

    def download(self, tick: int):
        """(header words uint32[16], off uint32[30][8], cnt uint32[30][8], row table uint32[n_rows]) of one tick as it
        stands on the device (rgb_train_plan_download; synchronises)."""
        raw = np.zeros(496, dtype=np.uint32)                      # sizeof(rgb_train_tick) = 1984
        rows = np.zeros(max(self.blocks_per_tick // 8, 1), dtype=np.uint32)
        n = self.eng._L.rgb_train_plan_download(self.eng._h, self.h, tick, raw.ctypes.data, rows.ctypes.data, len(rows))
        if n < 0:
            raise RgbError(n, "rgb_train_plan_download")
        return raw[:16].copy(), raw[16:256].reshape(30, 8).copy(), raw[256:496].reshape(30, 8).copy(), rows[:n].copy()

    def build_device(self, first_tick: int, n_ticks: int, d_bucket_counts: int, stream: int = 0):
        """Ticks [first_tick, first_tick + n_ticks) from uint32[n_ticks][TRAIN_BUCKETS] in DEVICE memory, one kernel
        on `stream` (rgb_train_plan_build_device): nothing of the plan passes through the host."""
        self.eng._check(self.eng._L.rgb_train_plan_build_device(self.eng._h, self.h, first_tick, n_ticks, d_bucket_counts,
                                                                stream or None), "rgb_train_plan_build_device")

    def fit(self, first_tick: int, n_ticks: int, stream: int = 0):
        """Tell the host the rows of the built ticks (rgb_train_plan_fit: 4 bytes per tick come back; synchronises):
        launches over them take a grid of their rows instead of the rows bound."""
        self.eng._check(self.eng._L.rgb_train_plan_fit(self.eng._h, self.h, first_tick, n_ticks, stream or None), "rgb_train_plan_fit")
        self.blocks_per_tick = int(self.eng._L.rgb_train_plan_blocks_per_tick(self.h))

    def close(self):
        if self.h:
            self.eng._L.rgb_train_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def train_bucket(kind, flags, server, n_members):
    """rgb_train_bucket over numpy arrays: (class rank of the kind, group mod 8, success flag)."""
    rank = np.append(abi.KIND_RANK, 15).astype(np.uint32)[np.minimum(np.asarray(kind), abi.N_KINDS)]   # unknown: NOP
    shard = (np.asarray(server, dtype=np.uint32) // n_members) & 7
    return (rank * 8 + shard) * 2 + (np.asarray(flags, dtype=np.uint32) & 1)


def wal_layout(records: np.ndarray, base: int = 0) -> int:
    """Fill out_offset for back-to-back records from `base`; returns the end offset (host helper)."""
    assert records.dtype == abi.WAL_RECORD_DTYPE and records.flags["C_CONTIGUOUS"]
    return int(lib().rgb_wal_layout(records.ctypes.data if len(records) else None, len(records), base))


def wal_batch_bound(cmds, writers, file, data_bytes: int):
    """(bytes of `out`, event rows, pairs) that always suffice for a WAL batch call -- host helper, no device work;
    RgbError(RGB_E_INVAL) for what the batch calls refuse."""
    cmds = np.ascontiguousarray(cmds, dtype=abi.WAL_CMD_DTYPE)
    writers = np.ascontiguousarray(writers, dtype=abi.WAL_WRITER_DTYPE)
    file = np.ascontiguousarray(file, dtype=abi.WAL_FILE_DTYPE).reshape(1)
    out, ev, rg = C.c_uint64(0), C.c_uint32(0), C.c_uint32(0)
    rc = lib().rgb_wal_batch_bound(cmds.ctypes.data if len(cmds) else None, len(cmds),
                                   writers.ctypes.data if len(writers) else None, len(writers), file.ctypes.data,
                                   data_bytes, C.byref(out), C.byref(ev), C.byref(rg))
    if rc != 0:
        raise RgbError(rc, "rgb_wal_batch_bound")
    return out.value, ev.value, rg.value


def wal_scan(file_bytes, cap: int | None = None):
    """recover_records/5's record walk over a whole WAL file (host code, no device):
    (records as abi.WAL_SCANNED_DTYPE, consumed bytes, end reason abi.WAL_END_*)."""
    buf = np.frombuffer(bytes(file_bytes), dtype=np.uint8) if not isinstance(file_bytes, np.ndarray) else \
        np.ascontiguousarray(file_bytes, dtype=np.uint8)
    n, consumed, end = C.c_uint32(0), C.c_uint64(0), C.c_uint32(0)
    if cap is None:                                   # count first, then size the array
        rc = lib().rgb_wal_scan(buf.ctypes.data if len(buf) else None, len(buf), None, 0,
                                C.byref(n), C.byref(consumed), C.byref(end))
        if rc != 0:
            raise RgbError(rc, "rgb_wal_scan")
        cap = max(1, n.value)
    out = np.zeros(cap, dtype=abi.WAL_SCANNED_DTYPE)
    rc = lib().rgb_wal_scan(buf.ctypes.data if len(buf) else None, len(buf), out.ctypes.data, cap,
                            C.byref(n), C.byref(consumed), C.byref(end))
    if rc != 0:
        raise RgbError(rc, "rgb_wal_scan")
    return out[:n.value].copy(), consumed.value, end.value


def segment_layout(entries: np.ndarray, max_count: int = 4096):
    """(DataOffset of every payload, file size) of a segment with MaxCount index records (host helper)."""
    entries = np.ascontiguousarray(entries, dtype=abi.SEG_ENTRY_DTYPE)
    offs = np.zeros(len(entries), dtype=np.uint64)
    size = lib().rgb_segment_layout(entries.ctypes.data if len(entries) else None, len(entries), max_count,
                                    offs.ctypes.data if len(entries) else None)
    return offs, int(size)


def snapshot_layout(items: np.ndarray, base: int = 0):
    """(a copy of `items` with out_offset filled back to back from `base`, the offset behind the last image)"""
    items = np.ascontiguousarray(items, dtype=abi.SNAP_ITEM_DTYPE).copy()
    end = lib().rgb_snapshot_layout(items.ctypes.data if len(items) else None, len(items), base)
    return items, int(end)


def _compact_args(sources, live):
    """(sources as abi.SEG_SOURCE_DTYPE, the live list as a flat uint64 array or None, its number of pairs)"""
    sources = np.ascontiguousarray(sources, dtype=abi.SEG_SOURCE_DTYPE)
    if live is None:
        return sources, None, 0
    live = np.ascontiguousarray(live, dtype=np.uint64).reshape(-1)
    if len(live) % 2:
        raise ValueError("the live list is (first, last) pairs")
    # an empty list is still a list ("nothing is live"), so it keeps a pointer
    return sources, (live if len(live) else np.zeros(2, dtype=np.uint64)), len(live) // 2


def segment_compact_bound(sources, live, files_bytes: int):
    """(a size that always holds the compacted image, MaxCount = the number of live indexes) -- host helper, no
    device work; RgbError(RGB_E_INVAL) for malformed descriptors, as the compact calls answer them."""
    sources, live, n_live = _compact_args(sources, live)
    bound, max_count = C.c_uint64(0), C.c_uint32(0)
    rc = lib().rgb_segment_compact_bound(sources.ctypes.data if len(sources) else None, len(sources),
                                         live.ctypes.data if live is not None else None, n_live, files_bytes,
                                         C.byref(bound), C.byref(max_count))
    if rc != 0:
        raise RgbError(rc, "rgb_segment_compact_bound")
    return int(bound.value), int(max_count.value)


def segment_compact_select(members, segrefs, live, sizing: bool = False):
    """The fold of major_compaction/3 and minor_compaction/2 for many members (host helper, no device work): `members`
    as abi.SEG_MEMBER_DTYPE, `segrefs` (range_first, range_last) pairs newest first, `live` pairs.  -> (one
    abi.SEG_PICK_DTYPE row per segref, the selected pairs as an (n, 2) uint64 array); sizing: the number of pairs."""
    members = np.ascontiguousarray(members, dtype=abi.SEG_MEMBER_DTYPE)
    segrefs = np.ascontiguousarray(segrefs, dtype=np.uint64).reshape(-1)
    live = np.ascontiguousarray(live if live is not None else [], dtype=np.uint64).reshape(-1)
    if len(segrefs) % 2 or len(live) % 2:
        raise ValueError("segrefs and the live list are (first, last) pairs")
    n_out = C.c_uint32(0)
    args = (members.ctypes.data if len(members) else None, len(members), segrefs.ctypes.data if len(segrefs) else None,
            len(segrefs) // 2, live.ctypes.data if len(live) else None, len(live) // 2)
    rc = lib().rgb_segment_compact_select(*args, None, None, 0, C.byref(n_out))
    if rc != 0:
        raise RgbError(rc, "rgb_segment_compact_select")
    if sizing:
        return int(n_out.value)
    picks = np.zeros(len(segrefs) // 2, dtype=abi.SEG_PICK_DTYPE)
    out = np.zeros((max(1, n_out.value), 2), dtype=np.uint64)
    rc = lib().rgb_segment_compact_select(*args, picks.ctypes.data, out.ctypes.data, n_out.value, C.byref(n_out))
    if rc != 0:
        raise RgbError(rc, "rgb_segment_compact_select")
    return picks, out[:n_out.value]


def segment_compact_take_groups(members, infos, num_live, max_count: int = abi.SEG_MAX_ENTRIES,
                                max_size: int = abi.SEG_MAX_SIZE_B):
    """compaction_groups/3 with take_group/3 per member (host helper): `members` as abi.SEG_TAKE_MEMBER_DTYPE (src_first,
    src_n), `infos` (abi.SEG_INFO_DTYPE) and `num_live` per source, oldest first.  -> (members with n_groups and status
    filled in, the group ordinal of every source or abi.SEG_GROUP_NONE)."""
    members = np.ascontiguousarray(members, dtype=abi.SEG_TAKE_MEMBER_DTYPE).copy()
    infos = np.ascontiguousarray(infos, dtype=abi.SEG_INFO_DTYPE)
    num_live = np.ascontiguousarray(num_live, dtype=np.uint64)
    if len(num_live) != len(infos):
        raise ValueError("one num_live per info row")
    group_of = np.full(max(1, len(infos)), abi.SEG_GROUP_NONE, dtype=np.uint32)
    rc = lib().rgb_segment_compact_take_groups(members.ctypes.data if len(members) else None, len(members),
                                               infos.ctypes.data if len(infos) else None,
                                               num_live.ctypes.data if len(infos) else None, len(infos), max_count,
                                               max_size, group_of.ctypes.data)
    if rc != 0:
        raise RgbError(rc, "rgb_segment_compact_take_groups")
    return members, group_of[:len(infos)]


def segment_compact_groups_bound(groups, sources, live, files_bytes: int):
    """(a copy of `groups` with out_offset / out_bytes laid out back to back, the bytes of `out` in all, MaxCount per
    group) -- host helper, no device work; RgbError(RGB_E_INVAL) for what the batched compact calls refuse."""
    groups = np.ascontiguousarray(groups, dtype=abi.SEG_GROUP_DTYPE).copy()
    sources, live, n_live = _compact_args(sources, live)
    total = C.c_uint64(0)
    counts = np.zeros(max(1, len(groups)), dtype=np.uint32)
    rc = lib().rgb_segment_compact_groups_bound(groups.ctypes.data if len(groups) else None, len(groups),
                                                sources.ctypes.data if len(sources) else None, len(sources),
                                                live.ctypes.data if live is not None else None, n_live, files_bytes,
                                                C.byref(total), counts.ctypes.data)
    if rc != 0:
        raise RgbError(rc, "rgb_segment_compact_groups_bound")
    return groups, int(total.value), counts[:len(groups)]


def segment_flush_bound(writers, n_entries: int, data_bytes: int):
    """(bytes of `out`, piece rows) that always suffice for a flush call -- host helper, no device work;
    RgbError(RGB_E_INVAL) for malformed writers, as the flush calls answer them."""
    writers = np.ascontiguousarray(writers, dtype=abi.SEG_WRITER_DTYPE)
    out_bound, pieces_bound = C.c_uint64(0), C.c_uint32(0)
    rc = lib().rgb_segment_flush_bound(writers.ctypes.data if len(writers) else None, len(writers), n_entries,
                                       data_bytes, C.byref(out_bound), C.byref(pieces_bound))
    if rc != 0:
        raise RgbError(rc, "rgb_segment_flush_bound")
    return int(out_bound.value), int(pieces_bound.value)


def segment_scan(file_bytes, cap: int | None = None):
    """read_header/1 and the index walk over a whole segment file (host code, no device):
    (records as abi.SEG_ENTRY_DTYPE, version, max_count, end reason abi.SEG_END_*)."""
    buf = np.frombuffer(bytes(file_bytes), dtype=np.uint8) if not isinstance(file_bytes, np.ndarray) else \
        np.ascontiguousarray(file_bytes, dtype=np.uint8)
    n, ver, mc, end = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    ptr = buf.ctypes.data if len(buf) else None
    if cap is None:
        rc = lib().rgb_segment_scan(ptr, len(buf), None, 0, C.byref(n), C.byref(ver), C.byref(mc), C.byref(end))
        if rc != 0:
            raise RgbError(rc, "rgb_segment_scan")
        cap = max(1, n.value)
    out = np.zeros(cap, dtype=abi.SEG_ENTRY_DTYPE)
    rc = lib().rgb_segment_scan(ptr, len(buf), out.ctypes.data, cap, C.byref(n), C.byref(ver), C.byref(mc),
                                C.byref(end))
    if rc != 0:
        raise RgbError(rc, "rgb_segment_scan")
    return out[:n.value].copy(), ver.value, mc.value, end.value


def combine_checksums(per_server: np.ndarray, first: int = 0) -> int:
    """The host-side 'checksum of checksums' rgb_state_checksum returns."""
    acc = 0
    for k, c in enumerate(per_server.tolist()):
        acc = (acc + c * (2 * (first + k) + 1)) & 0xFFFFFFFFFFFFFFFF
    return acc
